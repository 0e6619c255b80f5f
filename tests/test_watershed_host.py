"""CPU: the numpy restatements of the watershed rule (ws_ref.py) -- the heap on (M, D) with the labels in key order against the literal
random-order relaxation of both passes (and its whole-volume sweeps, the fast form the GPU tests use), voxel for voxel; M against the reconstruction by erosion of the merged morphological rule
(morph_ref.py); every region C-connected around its marker; the closed forms of a plateau and of a basin behind a pass; the ctypes mirrors
of the structs against the header text; the Python-side size checks; the usage errors and the help of advantra_cli --watershed (caught
before a device is opened)."""
import ctypes as C
import os
import re
import subprocess
import numpy as np
import pytest
from pnr_amd import lib
import ws_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "pnr_amd", "host", "advantra_cli")
SHAPES = [(3, 5, 7), (1, 9, 11), (2, 2, 2), (4, 4, 5), (1, 1, 6)]


def sid(s):
    return "x".join(map(str, s))


def stack(shape, levels, seed):
    """a random stack with `levels` grey levels, a mask with holes (thr 1: the zeros) and a few random markers, some of them in the holes"""
    rng = np.random.default_rng(seed)
    grey = np.linspace(40, 255, levels).astype(np.uint8)
    V = grey[rng.integers(0, levels, shape)]
    V[rng.random(shape) < 0.25] = 0
    relief = grey[rng.integers(0, levels, shape)] if seed % 2 else None
    mark = np.zeros(shape, np.int32)
    n = max(2, V.size // 12)
    at = rng.choice(V.size, n, replace=False)
    mark.ravel()[at] = rng.integers(1, 5, n)
    return V, relief, mark


@pytest.mark.parametrize("shape", SHAPES, ids=sid)
def test_the_heap_equals_the_random_order_relaxation(shape):
    for levels in (2, 3, 4, 256):
        for seed in range(3):
            V, relief, mark = stack(shape, levels, 10 * levels + seed)
            for C_ in ref.CONNS:
                ia, La, Ma, Ka = ref.run(V, 1, C_, relief, markers=mark)
                for order in (1, 2):
                    ib, Lb, Mb, Kb = ref.run(V, 1, C_, relief, markers=mark, solver=lambda *a: ref.flood_relax(*a, seed=order))
                    assert np.array_equal(Ka, Kb) and np.array_equal(La, Lb) and np.array_equal(Ma, Mb) and ia == ib, (shape, levels, seed, C_)
                ic, Lc, Mc, Kc = ref.run(V, 1, C_, relief, markers=mark, solver=ref.flood_sweeps)
                assert np.array_equal(Ka, Kc) and np.array_equal(La, Lc) and ia == ic, (shape, levels, seed, C_)
                assert ia["n_dropped"] == int(((mark > 0) & (V < 1)).sum()) and ia["n_reached"] + ia["n_unreached"] == ia["n_mask"]


@pytest.mark.parametrize("shape", SHAPES, ids=sid)
def test_the_level_is_the_reconstruction_by_erosion_and_regions_hold_their_markers(shape):
    for levels in (2, 4, 256):
        V, relief, mark = stack(shape, levels, 100 + levels)
        for C_ in ref.CONNS:
            mask, R, mk, t, _ = ref.setup(V, 1, relief, markers=mark)
            info, L, M, K = ref.run(V, 1, C_, relief, markers=mark)
            E, conn = ref.minimax(mask, R, mk, C_)
            reached = K != ref.INF
            assert np.array_equal(reached, conn & mask), (shape, levels, C_)
            assert np.array_equal(M[reached], E[reached]), (shape, levels, C_)
            assert ((L > 0) == reached).all() and np.array_equal(L[mk > 0], mk[mk > 0])
            assert ref.regions_hold_their_markers(L, mk, C_), (shape, levels, C_)
            one = np.where(mk > 0, np.arange(1, mk.size + 1).reshape(mk.shape), 0)  # a label per marker voxel: regions in the strict sense
            _, L1, M1, _ = ref.run(V, 1, C_, relief, markers=one)
            assert np.array_equal(M1, M) and ref.regions_hold_their_markers(L1, one, C_), (shape, levels, C_)


def test_a_plateau_gives_the_step_count_and_the_smaller_label_on_a_tie():
    V = np.full((1, 1, 9), 100, np.uint8)
    mark = np.zeros(V.shape, np.int32)
    mark[0, 0, 0], mark[0, 0, 8] = 7, 3
    info, L, M, K = ref.run(V, 0, 4, markers=mark)
    assert (K[0, 0] & ref.DSAT).tolist() == [0, 1, 2, 3, 4, 3, 2, 1, 0] and (M == 155).all()
    assert L[0, 0].tolist() == [7, 7, 7, 7, 3, 3, 3, 3, 3] and info["d_max"] == 4 and info["n_regions"] == 2


def test_a_basin_behind_a_pass_keeps_the_pass_height_and_restarts_the_count():
    relief = np.array([[[10, 10, 50, 20, 5, 5, 90, 0]]], np.uint8)
    V = np.full(relief.shape, 9, np.uint8)
    info, L, M, K = ref.run(V, 0, 4, relief, points=[[0, 0, 0]])
    assert M[0, 0].tolist() == [10, 10, 50, 50, 50, 50, 90, 90] and (K[0, 0] & ref.DSAT).tolist() == [0, 1, 1, 2, 3, 4, 1, 2]
    assert (L == 1).all() and info["m_max"] == 90 and info["d_max"] == 4


def test_one_key_with_the_label_in_its_low_bits_would_be_wrong():
    """the example behind the two passes: across a rise both candidates become (R(t), 1, .); the rule takes the label of the tight
    neighbour with the smallest LABEL, not of the one with the smallest key"""
    relief = np.array([[[0, 0, 9, 0]]], np.uint8)
    V = np.full(relief.shape, 9, np.uint8)
    mark = np.array([[[5, 0, 0, 2]]], np.int32)
    _, L, M, K = ref.run(V, 0, 4, relief, markers=mark)
    assert L[0, 0].tolist() == [5, 5, 2, 2] and (K[0, 0, 2] >> 24, K[0, 0, 2] & ref.DSAT) == (9, 1)  # from (0, 1, 5) and from (0, 0, 2): both tight


def test_points_duplicates_and_drops():
    V = np.full((2, 3, 4), 50, np.uint8)
    V[0, 0, 0] = 0
    pts = [[1, 1, 1], [1.2, 0.8, 1.4], [0, 0, 0], [np.nan, 0, 0], [3, 2, 0]]
    info, L, _, _ = ref.run(V, 1, 6, points=pts, labels=[9, 4, 1, 1, 6])
    assert info["n_dropped"] == 2 and info["n_marker_vox"] == 2 and L[1, 1, 1] == 4 and L[0, 2, 3] == 6 and L[0, 0, 0] == 0
    assert set(np.unique(L)) == {0, 4, 6}


def test_struct_layout_matches_header():
    hdr = open(os.path.join(ROOT, "include", "pnr_hip.h")).read()
    ctype = {"int32_t": C.c_int32, "int64_t": C.c_int64}

    def fields(name):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), hdr, re.S).group(1)
        out = []
        for decl in filter(None, (d.strip() for d in body.split(";"))):
            m = re.match(r"(\w+)\s*(.*)", decl)
            out += [(n.strip(), ctype[m.group(1)]) for n in m.group(2).split(",")]
        return out

    assert fields("pnr_watershed_opts") == list(lib.WatershedOpts._fields_)
    assert fields("pnr_watershed_info") == list(lib.WatershedInfo._fields_)
    assert C.sizeof(lib.WatershedOpts) == 8 and C.sizeof(lib.WatershedInfo) == 104
    assert "pnr_watershed" in lib.PRODUCT_EXPORTS and re.search(r"^int pnr_watershed\(", hdr, re.M) and hasattr(lib.load(), "pnr_watershed")
    assert set(ref.EXACT) < {f for f, _ in lib.WatershedInfo._fields_}
    assert ref.tile() == __import__("morph_ref").tile()  # the morph tile


def test_sizes_are_checked_before_the_call():
    class Fake(lib.Context):
        def __init__(self):
            self.shape, self.h, self.L = (2, 3, 4), None, None  # (no library call is reached)

        def close(self):
            pass

    with pytest.raises(ValueError, match="marker volume of 23 voxels for a volume of 24"):
        Fake().watershed(markers=np.zeros(23, np.int32))
    with pytest.raises(ValueError, match="relief of 25 voxels for a volume of 24"):
        Fake().watershed(points=[[0, 0, 0]], relief=np.zeros(25, np.uint8))
    with pytest.raises(ValueError, match="2 labels for 1 points"):
        Fake().watershed(points=[[0, 0, 0]], labels=[1, 2])
    with pytest.raises(ValueError, match="1 labels for 0 points"):
        Fake().watershed(markers=np.zeros(24, np.int32), labels=[1])


def _cli(*args):
    return subprocess.run([CLI, *args], capture_output=True, text=True, timeout=60)


W = ("--watershed", "-i", "x.raw", "--labels", "o.raw")
SWC = ("--markers-swc", "t.swc")
TRACE = ("-f", "advantra_func", "-i", "x.raw", "-p", "2,3", "0", "5", "0.3", "3", "2", "40", "50", "2", "4", "5")


@pytest.mark.parametrize("args,msg", [
    (W, "--watershed needs one of --markers-swc and --markers"), ((*W, *SWC, "--markers", "m.raw"), "--markers-swc and --markers: one of them"),
    (("--watershed", "-i", "x.raw", *SWC), "--watershed needs --labels OUT.raw"), (("--watershed", "--labels", "o.raw", *SWC), "--watershed needs -i"),
    ((*W, "--markers-swc"), "--markers-swc FILE.swc"), ((*W, "--markers", "m.txt"), "--markers FILE.raw"), ((*W, "--markers"), "--markers FILE.raw"), ((*W, *SWC, "--markers-by", "x"), "--markers-by tree|node"),
    ((*W, *SWC, "--markers-by"), "--markers-by tree|node"), ((*W, "--markers", "m.raw", "--markers-by", "node"), "--markers-by needs --markers-swc"),
    ((*W, *SWC, "--relief"), "--relief FILE.raw"), ((*W, *SWC, "--levels"), "--levels OUT.raw"), ((*W, "--labels"), "--labels OUT.raw"),
    ((*W, *SWC, "--connectivity", "5"), "--connectivity"), ((*W, *SWC, "--threshold", "300"), "--threshold"),
    (("-i", "x.raw", "--labels", "o.raw"), "need --components"), (("-i", "x.raw", *SWC), "--levels need --watershed -i stack"),
    (("-i", "x.raw", "--markers", "m.raw"), "need --watershed"), (("-i", "x.raw", "--relief", "r.raw"), "need --watershed"),
    (("-i", "x.raw", "--levels", "l.raw"), "need --watershed"), (("-i", "x.raw", "--markers-by", "node"), "need --watershed"),
    (("--components", "-i", "x.raw", "--connectivity", "8"), "--connectivity 6|26"), ((*W, *SWC, "--min-size", "3"), "--watershed: not with"),
    ((*W, *SWC, "--per-component", "c.csv"), "--watershed: not with"), ((*W, *SWC, "--zscale", "2"), "need --distance"),
    ((*W, *SWC, "--skeleton"), "--skeleton: not with"), ((*W, *SWC, "--morph"), "--morph: not with"), ((*W, *SWC, "--edt"), "--watershed: not with"),
    ((*W, *SWC, "--components"), "--watershed: not with"), ((*W, *SWC, "--info"), "--watershed: not with"),
    (("--watershed", "--labels", "o.raw", *SWC, *TRACE), "--watershed: not with")])
def test_cli_usage_errors(args, msg):
    r = _cli(*args, "-g", "99") if "-p" not in args else _cli("-g", "99", *args)  # (a device that does not exist: the error comes first)
    assert r.returncode == 1 and msg in r.stderr and r.stderr.count("\n") == 1, (args, r.stderr)


def test_cli_help_lists_the_flags():
    r = _cli("--help")
    assert r.returncode == 0
    for flag in ("--watershed -i stack", "--markers-swc FILE.swc", "--connectivity 4|8|6|26", "--connectivity 6|26", "--markers-by tree|node", "--markers FILE.raw", "--relief FILE.raw", "--labels OUT.raw", "--levels OUT.raw"):
        assert flag in r.stdout, flag
