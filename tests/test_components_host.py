"""CPU: the numpy restatement of the connected-component rule (components_ref.py) against scipy.ndimage.label where scipy is present,
the ctypes mirrors of the component structs against the header text, and the usage errors of advantra_cli --components / --despeckle
(caught before a device is opened)."""
import ctypes as C
import os
import re
import subprocess
import numpy as np
import pytest
from pnr_amd import lib
import components_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "pnr_amd", "host", "advantra_cli")


def _inputs():
    rng = np.random.default_rng(7)
    shape = (9, 17, 67)
    l, h, w = shape
    z, y, x = np.meshgrid(np.arange(l), np.arange(h), np.arange(w), indexing="ij")
    out = {"zero": np.zeros(shape, bool), "full": np.ones(shape, bool), "checker": ((x + y + z) & 1) == 0, "diagonal": (x == y) & (y == z),
           "rows": ((y & 1) == 0) & ((z & 1) == 0), "plane": np.broadcast_to(rng.random((1, h, w)) < 0.4, (1, h, w)).copy()}
    for d in (0.05, 0.10, 0.31, 0.6):
        out["rand%02d" % round(100 * d)] = rng.random(shape) < d
    return out


@pytest.mark.parametrize("conn", [6, 26])
@pytest.mark.parametrize("kind", sorted(_inputs()))
def test_reference_against_scipy(kind, conn):
    ndimage = pytest.importorskip("scipy.ndimage")
    F = _inputs()[kind]
    V = np.where(F, 200, 3).astype(np.uint8)
    info, labels, comps = ref.label(V, 128, conn)
    theirs, n = ndimage.label(F, ndimage.generate_binary_structure(3, 1 if conn == 6 else 3))
    assert n == info["n_comp"] == len(comps)
    flat = theirs.ravel()
    ids, first = np.unique(flat, return_index=True)  # renumbered by first voxel
    ids, first = ids[ids > 0], first[ids > 0]
    remap = np.zeros(n + 1, np.int32)
    remap[ids[np.argsort(first)]] = np.arange(1, n + 1)
    assert np.array_equal(remap[theirs], labels)
    assert np.array_equal(comps["first"], np.sort(first)) and np.array_equal(comps["size"], np.bincount(labels.ravel(), minlength=n + 1)[1:])
    if n:
        com = np.array(ndimage.center_of_mass(F, labels, np.arange(1, n + 1)))  # (z, y, x)
        assert np.allclose(com[:, 2], comps["sx"] / comps["size"]) and np.allclose(com[:, 0], comps["sz"] / comps["size"])
        boxes = ndimage.find_objects(labels)
        assert all(b[2].start == c["x0"] and b[2].stop - 1 == c["x1"] and b[0].start == c["z0"] and b[1].stop - 1 == c["y1"] for b, c in zip(boxes, comps))


def test_reference_min_size_threshold_and_despeckle():
    rng = np.random.default_rng(3)
    V = rng.integers(0, 256, (4, 9, 11)).astype(np.uint8)
    full = ref.label(V, 200, 6)
    info, labels, comps = ref.label(V, 200, 6, 3)
    keep = full[2]["size"] >= 3
    assert comps.tobytes() == full[2][keep].tobytes() and info["n_small"] == int((~keep).sum()) > 0 and info["vox_small"] == int(full[2]["size"][~keep].sum())
    assert np.array_equal(np.unique(labels), np.arange(info["n_comp"] + 1)) and info["largest"] == comps["size"].max()
    out, dinfo = ref.despeckle(V, 3, 200, 6)
    assert dinfo == info and np.array_equal(out == V, ~((V >= 200) & (labels == 0)))
    assert ref.threshold(V) == int(V.astype(np.int64).sum()) // V.size and ref.threshold(np.zeros((1, 2, 2), np.uint8)) == 1 and ref.threshold(V, 0) == 0
    assert ref.label(V, 0, 6)[0]["n_comp"] == 1


def test_struct_layout_matches_header():
    hdr = open(os.path.join(ROOT, "include", "pnr_hip.h")).read()
    ctype = {"int32_t": C.c_int32, "int64_t": C.c_int64}

    def fields(name):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), hdr, re.S).group(1)
        out = []
        for decl in filter(None, (d.strip() for d in body.split(";"))):
            t, names = decl.split(None, 1)
            out += [(n.strip(), ctype[t]) for n in names.split(",")]
        return out

    assert fields("pnr_components_opts") == list(lib.ComponentsOpts._fields_)
    assert fields("pnr_components_info") == list(lib.ComponentsInfo._fields_)
    want = fields("pnr_component")
    assert [n for n, _ in want] == list(lib.COMPONENT_DT.names) == list(ref.COMPONENT_DT.names)
    assert all(lib.COMPONENT_DT[n].itemsize == C.sizeof(t) and lib.COMPONENT_DT[n].kind == "i" for n, t in want)
    assert C.sizeof(lib.ComponentsOpts) == 16 and C.sizeof(lib.ComponentsInfo) == 56 and lib.COMPONENT_DT.itemsize == 80 == ref.COMPONENT_DT.itemsize
    assert lib.COMPONENT_DT == ref.COMPONENT_DT
    for name in ("pnr_label_components", "pnr_despeckle_volume"):
        assert name in lib.PRODUCT_EXPORTS and re.search(r"^int %s\(" % name, hdr, re.M)


def test_tile_constants_are_where_the_tests_read_them():
    txt = open(os.path.join(ROOT, "pnr_amd", "csrc", "components.h")).read()
    got = dict(re.findall(r"constexpr int (CC_TX|CC_TY|CC_TZ) = (\d+);", txt))
    assert sorted(got) == ["CC_TX", "CC_TY", "CC_TZ"] and all(int(v) >= 1 for v in got.values())


def _cli(*args):
    return subprocess.run([CLI, *args], capture_output=True, text=True, timeout=60)


@pytest.mark.parametrize("args,msg", [
    (("--despeckle", "0"), "--despeckle MIN"), (("--despeckle", "x"), "--despeckle MIN"), (("--despeckle", "5,256"), "--despeckle MIN"),
    (("--despeckle", "5,-1,18"), "--despeckle MIN"), (("--despeckle", "5,1,6,2"), "--despeckle MIN"), (("--despeckle",), "--despeckle MIN"),
    (("--components", "--connectivity", "18"), "--connectivity 6|26"), (("--components", "--threshold", "256"), "--threshold T"),
    (("--components", "--threshold", "-2"), "--threshold T"), (("--components", "--min-size", "0"), "--min-size M"),
    (("--components", "--labels", "out.tif"), "--labels OUT.raw"), (("--components",), "--components needs -i"),
    (("--min-size", "3"), "need --components"), (("--components", "-i", "x.raw", "--despeckle", "3"), "--components: not with"),
    (("--despeckle", "3", "--info", "-i", "x.raw"), "--despeckle needs a tracing run")])
def test_cli_usage_errors(args, msg):
    r = _cli(*args, "-g", "99")  # (a device that does not exist: the error comes first)
    assert r.returncode == 1 and msg in r.stderr, (args, r.stderr)


def test_cli_help_lists_the_flags():
    r = _cli("--help")
    assert r.returncode == 0
    for flag in ("--despeckle MIN[,THR[,CONN]]", "--components -i stack", "--threshold T", "--connectivity 6|26", "--min-size M", "--labels OUT.raw", "--per-component FILE.csv"):
        assert flag in r.stdout, flag
