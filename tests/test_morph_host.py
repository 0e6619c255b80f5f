"""CPU: the numpy restatement of the morphological reconstruction rule (morph_ref.py) -- the literal recursion against the max-heap
widest-path solver, bit for bit, the threshold decomposition of the grey fill against scipy.ndimage.binary_fill_holes where scipy is
present, the bounds of the rule, the hollow soma that is the reason for the feature (thin_ref.py), the ctypes mirrors of the structs against
the header text, the Python-side marker check and the usage errors of advantra_cli's morphology flags (caught before a device is opened)."""
import ctypes as C
import os
import re
import subprocess
import numpy as np
import pytest
from pnr_amd import lib
import morph_ref as ref
import thin_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "pnr_amd", "host", "advantra_cli")
SHAPES = [(3, 7, 9), (1, 12, 13), (2, 2, 2), (4, 5, 6), (1, 1, 5)]
KINDS = ("rand", "smooth", "steps")


def sid(s):
    return "x".join(map(str, s))


@pytest.mark.parametrize("shape", SHAPES, ids=sid)
def test_the_recursion_equals_the_widest_path(shape):
    for kind in KINDS:
        V = ref.volume(shape, kind)
        for C_ in ref.CONNS:
            for name, M in ref.markers(V).items():
                for op in ("dilate", "erode"):
                    a, _ = ref.run(V, op, M, C=C_)
                    b, _ = ref.run(V, op, M, C=C_, solver=ref.dilate_heap)
                    assert a.dtype == np.uint8 and np.array_equal(a, b), (shape, kind, C_, name, op)
            for op, h in (("fill", 0), ("hmax", 1), ("hmax", 40), ("hdome", 40), ("hdome", 255)):
                a, _ = ref.run(V, op, h=h, C=C_)
                b, _ = ref.run(V, op, h=h, C=C_, solver=ref.dilate_heap)
                assert np.array_equal(a, b), (shape, kind, C_, op, h)


@pytest.mark.parametrize("shape", SHAPES, ids=sid)
def test_bounds_of_the_rule(shape):
    for kind in KINDS:
        V = ref.volume(shape, kind)
        for C_ in ref.CONNS:
            for M in ref.markers(V).values():
                R = ref.dilate(M, V, C_)
                assert (np.minimum(M, V) <= R).all() and (R <= V).all()
                E, _ = ref.run(V, "erode", M, C=C_)
                assert (E >= V).all() and (E <= np.maximum(M, V)).all()
            F, _ = ref.run(V, "fill", C=C_)
            assert (F >= V).all() and np.array_equal(ref.run(F, "fill", C=C_)[0], F)  # never lowers a voxel; idempotent
            assert np.array_equal(F[ref.border(shape, C_)], V[ref.border(shape, C_)])
            for h in (1, 40, 255):
                D, _ = ref.run(V, "hdome", h=h, C=C_)
                H, _ = ref.run(V, "hmax", h=h, C=C_)
                assert (D <= h).all() and (H <= V).all() and np.array_equal(D, V - H)
    assert ref.run(V, "fill")[1] == 6 and ref.run(V, "hmax", h=3)[1] == 26


def test_connectivities_of_a_single_slice():
    V = ref.volume((1, 12, 13), "smooth")
    M = ref.markers(V)["rand"]
    assert np.array_equal(ref.dilate(M, V, 6), ref.dilate(M, V, 4)) and np.array_equal(ref.dilate(M, V, 26), ref.dilate(M, V, 8))
    V3 = ref.volume((3, 7, 9), "rand")
    M3 = ref.markers(V3)["rand"]
    for C_ in (4, 8):  # every slice on its own
        assert np.array_equal(ref.dilate(M3, V3, C_), np.stack([ref.dilate(M3[z:z + 1], V3[z:z + 1], C_)[0] for z in range(3)]))


@pytest.mark.parametrize("C_", (6, 26, 4, 8))
def test_fill_is_binary_fill_holes_at_every_threshold(C_):
    ndi = pytest.importorskip("scipy.ndimage")
    shape = (20, 23, 37) if C_ in (6, 26) else (1, 23, 37)
    V = ref.volume(shape, "smooth")
    F, _ = ref.run(V, "fill", C=C_)
    # a hole of {V >= t} is a component of its background that does not touch the border; the background's connectivity is C
    st = np.zeros((3, 3, 3), bool)
    for o in ref.offsets(C_):
        st[o[0] + 1, o[1] + 1, o[2] + 1] = True
    st[1, 1, 1] = True
    for t in range(1, 256):
        fg = V >= t
        if C_ in (6, 26):
            want = ndi.binary_fill_holes(fg, structure=st)
        else:
            want = ndi.binary_fill_holes(fg[0], structure=st[1])[None]
        assert np.array_equal(F >= t, want), (C_, t)


def test_hollow_kinds_tell_the_connectivities_apart():
    TZ, TY, TX = ref.tile()
    V = ref.volume((TZ + 5, 2 * TY + 3, TX + 7), "hollow")
    f6, f26 = ref.run(V, "fill", C=6)[0], ref.run(V, "fill", C=26)[0]
    assert f6[2, 3, 3] == 200 and f26[2, 3, 3] == 200  # the cavity inside one tile
    assert f6[TZ, TY, TX] == 200 and f26[TZ, TY, TX] == 200  # ... across a tile corner
    assert f6[2, TY + 7, 0] == 20 and f26[2, TY + 7, 0] == 20  # ... on the border: not filled
    assert f6[2, 3, 10] == 200 and f26[2, 3, 10] < 200  # ... open through a diagonal gap only


def test_the_hollow_soma_thins_to_a_curve_once_filled():
    V = ref.hollow_ball()
    F, _ = ref.run(V, "fill")
    t = 100
    before = thin_ref.skeletonize(V, t)[0]["n_skel"]
    after = thin_ref.skeletonize(F, t)[0]["n_skel"]
    assert 0 < after < before, (before, after)
    assert thin_ref.topology(V >= t) != thin_ref.topology(F >= t)
    # the background of the filled stack is one 6-component
    bg = 255 - np.where(F >= t, 255, 0).astype(np.uint8)
    seed = np.zeros(bg.shape, np.uint8)
    seed[0, 0, 0] = 255
    assert bg[0, 0, 0] == 255 and np.array_equal(ref.dilate(seed, bg, 6), bg)
    assert not np.array_equal(ref.dilate(seed, 255 - np.where(V >= t, 255, 0).astype(np.uint8), 6), 255 - np.where(V >= t, 255, 0).astype(np.uint8))


def test_struct_layout_matches_header():
    hdr = open(os.path.join(ROOT, "include", "pnr_hip.h")).read()
    ctype = {"int32_t": C.c_int32, "int64_t": C.c_int64, "uint64_t": C.c_uint64}

    def fields(name):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), hdr, re.S).group(1)
        out = []
        for decl in filter(None, (d.strip() for d in body.split(";"))):
            m = re.match(r"(\w+)\s*(.*)", decl)
            out += [(n.strip(), ctype[m.group(1)]) for n in m.group(2).split(",")]
        return out

    assert fields("pnr_morph_opts") == list(lib.MorphOpts._fields_)
    assert fields("pnr_morph_info") == list(lib.MorphInfo._fields_)
    assert C.sizeof(lib.MorphOpts) == 16 and C.sizeof(lib.MorphInfo) == 72
    for fn in ("pnr_morph_reconstruct", "pnr_morph_volume"):
        assert fn in lib.PRODUCT_EXPORTS and re.search(r"^int %s\(" % fn, hdr, re.M) and hasattr(lib.load(), fn)
    for name, v in lib.MORPH_OPS.items():
        assert int(re.search(r"#define PNR_MORPH_%s (\d+)" % name.upper(), hdr).group(1)) == v == ref.OPS[name]


def test_tile_constants_are_where_the_tests_read_them():
    assert len(ref.tile()) == 3 and all(v >= 2 for v in ref.tile())


def test_a_marker_of_the_wrong_size_is_refused_before_the_call():
    class Fake(lib.Context):
        def __init__(self):
            self.shape, self.h, self.L = (2, 3, 4), None, None  # (no library call is reached)

        def close(self):
            pass

    with pytest.raises(ValueError, match="marker of 23 voxels for a volume of 24"):
        Fake().morph_reconstruct(np.zeros(23, np.uint8), "dilate")
    with pytest.raises(ValueError, match="op 'open'"):
        Fake().morph_reconstruct(np.zeros(24, np.uint8), "open")
    with pytest.raises(ValueError, match="op 'close'"):
        Fake().morph_volume("close")


def _cli(*args):
    return subprocess.run([CLI, *args], capture_output=True, text=True, timeout=60)


M = ("--morph", "-i", "x.raw", "--morph-out", "o.raw")
TRACE = ("-f", "advantra_func", "-i", "x.raw", "-p", "2,3", "0", "5", "0.3", "3", "2", "40", "50", "2", "4", "5")


@pytest.mark.parametrize("args,msg", [
    ((*M, "--fill-holes", "x"), "--fill-holes 2d|3d"), ((*M, "--fill-holes"), "--fill-holes 2d|3d"), ((*M, "--hmax", "0"), "--hmax H"), ((*M, "--hmax", "256"), "--hmax H"),
    ((*M, "--hmax"), "--hmax H"), ((*M, "--hdome", "0"), "--hdome H"), ((*M, "--hdome", "x"), "--hdome H"), ((*M, "--hmax", "3", "--hdome", "3"), "--hmax and --hdome: one of them"),
    (("--morph", "-i", "x.raw", "--fill-holes", "3d"), "--morph needs --morph-out"), (("--morph", "--morph-out", "o.raw", "--fill-holes", "3d"), "--morph needs -i"),
    (M, "--morph needs one of --fill-holes, --hmax and --hdome"), (("--morph-out", "o.raw", "-i", "x.raw"), "--morph-out needs --morph"),
    ((*M, "--morph-out"), "--morph-out OUT"), ((*M, "--fill-holes", "3d", "--skeleton"), "--skeleton: not with"), ((*M, "--fill-holes", "3d", "--edt"), "--morph: not with"),
    ((*M, "--fill-holes", "3d", "--components"), "--morph: not with"), ((*M, "--fill-holes", "3d", "--despeckle", "3"), "--morph: not with"),
    ((*M, "--fill-holes", "3d", "--info"), "--morph: not with"), ((*M, "--fill-holes", "3d", "--distance", "a.swc", "b.swc"), "--morph: not with"),
    (("--morph", "--morph-out", "o.raw", "--hmax", "3", *TRACE), "--morph: not with")])
def test_cli_usage_errors(args, msg):
    r = _cli(*args, "-g", "99") if "-p" not in args else _cli("-g", "99", *args)  # (a device that does not exist: the error comes first)
    assert r.returncode == 1 and msg in r.stderr and r.stderr.count("\n") == 1, (args, r.stderr)


def test_cli_help_lists_the_flags():
    r = _cli("--help")
    assert r.returncode == 0
    for flag in ("--fill-holes 2d|3d", "--hmax H", "--hdome H", "--morph -i stack", "--morph-out OUT"):
        assert flag in r.stdout, flag
