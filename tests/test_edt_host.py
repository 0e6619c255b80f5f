"""CPU: the numpy restatement of the distance-transform rule (edt_ref.py) -- the literal rule against its separable form, bit for bit, and
against scipy.ndimage.distance_transform_edt where scipy is present --, the summary on hand-made stacks, the ctypes mirrors of the structs
against the header text, and the usage errors of advantra_cli --edt (caught before a device is opened)."""
import ctypes as C
import os
import re
import subprocess
import numpy as np
import pytest
from pnr_amd import lib
import edt_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "pnr_amd", "host", "advantra_cli")
SHAPES = [(5, 9, 11), (4, 7, 6), (1, 12, 13), (6, 6, 6), (3, 5, 5)]
DENSITIES = (0.1, 0.5, 0.9, 0.98, 1.0)
CAPS = (1, 3, 8, 64)


def _stack(shape, density, seed):
    rng = np.random.default_rng(seed)
    return np.where(rng.random(shape) < density, rng.integers(100, 256, shape), rng.integers(0, 100, shape)).astype(np.uint8)


@pytest.mark.parametrize("zd", [1.0, 1.5, 2.0, 3.3])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_literal_rule_equals_separable_form(shape, zd):
    for di, density in enumerate(DENSITIES):
        V = _stack(shape, density, 100 * SHAPES.index(shape) + di)
        assert density < 1.0 or (V >= 100).all()
        for rmax in CAPS:
            D, t = ref.transform(V, 100, zd, rmax)
            B = ref.brute(V, 100, zd, rmax)
            assert t == 100 and D.dtype == B.dtype == np.float32 and D.tobytes() == B.tobytes(), (shape, zd, density, rmax, int((D != B).sum()))
            assert ((D == 0) == (V < 100)).all() and D.max() <= rmax * rmax


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_reference_against_scipy(shape):
    ndimage = pytest.importorskip("scipy.ndimage")
    for di, density in enumerate(DENSITIES[:-1]):  # (scipy needs a background voxel)
        V = _stack(shape, density, 7 + di)
        if (V >= 100).all():
            continue
        theirs = np.rint(ndimage.distance_transform_edt(V >= 100) ** 2)
        for rmax in CAPS:
            D, _ = ref.transform(V, 100, 1.0, rmax)
            cap = rmax * rmax
            assert np.array_equal(D[D < cap], theirs[D < cap]) and (theirs[D == cap] >= cap).all(), (shape, density, rmax)


def test_info_on_hand_made_stacks():
    V = np.zeros((6, 8, 10), np.uint8)
    V[1:5, 2:6, 3:7] = 200  # an even-sided box: the maximum is attained at its 2 x 2 x 2 centre
    D, t = ref.transform(V, -1, 1.0, 64)
    assert t == max(1, int(V.astype(np.int64).sum()) // V.size)
    got = ref.info(V, D, t, 64)
    first = 4 + 10 * (3 + 8 * 2)
    assert int((D == D.max()).sum()) == 8 and D.max() == 4.0
    assert got == dict(n_vox=480, n_fg=64, n_capped=0, first_max=first, d2_max=4.0, thr_used=t, d_max=2.0, max_at=(4, 3, 2))
    Z = np.zeros((2, 3, 4), np.uint8)
    D, t = ref.transform(Z, -1, 2.0, 5)
    assert t == 1 and not D.any() and ref.info(Z, D, t, 5) == dict(n_vox=24, n_fg=0, n_capped=0, first_max=-1, d2_max=0.0, thr_used=1, d_max=0.0, max_at=None)
    O = np.full((2, 3, 4), 9, np.uint8)
    D, t = ref.transform(O, -1, 2.0, 5)
    assert t == 9 and (D == 25).all() and ref.info(O, D, t, 5) == dict(n_vox=24, n_fg=24, n_capped=24, first_max=0, d2_max=25.0, thr_used=9, d_max=5.0, max_at=(0, 0, 0))
    pts = np.array([[0, 0, 0], [3.4, 2.6, 0.5], [-7, 99, 0.49], [np.nan, 0, 0], [0, np.inf, 0]], np.float32)
    D, _ = ref.transform(V, 100, 1.0, 64)
    assert ref.at(D, pts).tolist() == [D[0, 0, 0], D[1, 3, 3], D[0, 7, 0], -1.0, -1.0]
    assert ref.threshold(V, 0) == 0 and ref.threshold(V, 255) == 255


def test_struct_layout_matches_header():
    hdr = open(os.path.join(ROOT, "include", "pnr_hip.h")).read()
    ctype = {"int32_t": C.c_int32, "int64_t": C.c_int64, "float": C.c_float}

    def fields(name):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), hdr, re.S).group(1)
        out = []
        for decl in filter(None, (d.strip() for d in body.split(";"))):
            t, names = decl.split(None, 1)
            out += [(n.strip(), ctype[t]) for n in names.split(",")]
        return out

    assert fields("pnr_edt_opts") == list(lib.EdtOpts._fields_)
    assert fields("pnr_edt_info") == list(lib.EdtInfo._fields_)
    assert C.sizeof(lib.EdtOpts) == 8 and C.sizeof(lib.EdtInfo) == 40
    assert "pnr_distance_transform" in lib.PRODUCT_EXPORTS and re.search(r"^int pnr_distance_transform\(", hdr, re.M)
    assert int(re.search(r"#define PNR_EDT_MAX_R (\d+)", hdr).group(1)) == lib.PNR_EDT_MAX_R == 1024


def test_tile_constants_are_where_the_tests_read_them():
    txt = open(os.path.join(ROOT, "pnr_amd", "csrc", "edt.h")).read()
    got = dict(re.findall(r"constexpr int (EDT_WX|EDT_ROWS|EDT_TPB) = (\d+);", txt))
    assert sorted(got) == ["EDT_ROWS", "EDT_TPB", "EDT_WX"] and all(int(v) >= 1 for v in got.values())


def _cli(*args):
    return subprocess.run([CLI, *args], capture_output=True, text=True, timeout=60)


@pytest.mark.parametrize("args,msg", [
    (("--edt",), "--edt needs -i"), (("--edt", "-i", "x.raw", "--edt-max", "0"), "--edt-max R"), (("--edt", "-i", "x.raw", "--edt-max", "1025"), "--edt-max R"),
    (("--edt", "-i", "x.raw", "--edt-max", "x"), "--edt-max R"), (("--edt", "-i", "x.raw", "--edt-max"), "--edt-max R"),
    (("--edt", "-i", "x.raw", "--edt-out", "d.tif"), "--edt-out OUT.raw"), (("--edt", "-i", "x.raw", "--edt-out"), "--edt-out OUT.raw"),
    (("--edt", "-i", "x.raw", "--at", "t.swc"), "go together"), (("--edt", "-i", "x.raw", "--per-node", "n.csv"), "go together"),
    (("--edt", "-i", "x.raw", "--threshold", "256"), "--threshold T"), (("--edt", "-i", "x.raw", "--zscale", "0.5"), "--zscale Z"),
    (("--edt-max", "3", "-i", "x.raw"), "need --edt"), (("--edt-out", "d.raw", "-i", "x.raw"), "need --edt"), (("--at", "t.swc", "-i", "x.raw"), "need --edt"),
    (("--edt", "--components", "-i", "x.raw"), "--edt: not with"), (("--edt", "-i", "x.raw", "--min-size", "3"), "need --components"),
    (("--edt", "-i", "x.raw", "--render-swc", "t.swc"), "--edt: not with"), (("--edt", "-i", "x.raw", "--distance", "a.swc", "b.swc"), "--edt: not with"),
    (("--edt", "-i", "x.raw", "--join-swc", "a.swc", "b.swc"), "--edt: not with"), (("--edt", "-i", "x.raw", "--info"), "--edt: not with"),
    (("--edt", "-i", "x.raw", "--despeckle", "3"), "--edt: not with"), (("--edt", "-i", "x.raw", "--measure-radius"), "--edt: not with"),
    (("--edt", "-f", "advantra_func", "-i", "x.raw", "-p", "2,3", "0", "5", "0.3", "3", "2", "40", "50", "2", "4", "5"), "--edt: not with")])
def test_cli_usage_errors(args, msg):
    r = _cli(*args, "-g", "99") if "-p" not in args else _cli("-g", "99", *args)  # (a device that does not exist: the error comes first)
    assert r.returncode == 1 and msg in r.stderr, (args, r.stderr)


def test_cli_help_lists_the_flags():
    r = _cli("--help")
    assert r.returncode == 0
    for flag in ("--edt -i stack", "--threshold T", "--edt-max R", "--zscale Z", "--edt-out OUT.raw", "--at tree.swc --per-node FILE.csv"):
        assert flag in r.stdout, flag
