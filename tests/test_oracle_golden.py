"""CPU: pin oracle/pnr_oracle.c against the golden vectors produced by the reference's own
frangi.cpp / seed.cpp (tests/golden/make_golden.py) and, on further inputs, against the
reference's outputs recorded in tests/golden/ref_cases.npz -- and live as well where oracle/_ref
is built.  Bit-exact: the restatement keeps the reference's operation order and precision."""
import ctypes as C
import os
import numpy as np
import pytest
import orc
import synth

REF_CASES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_cases.npz")
REF_RADII = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_radii.npz")


def references(ref, key, live, recorded=REF_CASES):
    """the reference's outputs for case `key`: as recorded in tests/golden/ref_cases.npz (make_golden.py ref_cases; or in `recorded`),
    and computed live by `live(ref)` where oracle/_ref is built"""
    with np.load(recorded) as z:
        out = [{k.split("__", 1)[1]: z[k] for k in z.files if k.startswith(key + "__")}]
    assert out[0], f"{key}: not in {recorded}"
    if ref is not None:
        out.append(live(ref))
    return out


def test_gaussian_matches_reference(oracle, golden):
    img = golden["img"]; l, h, w = img.shape
    F = np.zeros(img.shape, np.float32)
    oracle.orc_imgaussian3d(img, w, h, l, float(golden["sigs"][0]), float(golden["zdist"]), F)
    assert np.array_equal(F, golden["F_sig0"])


def test_hessian_matches_reference(oracle, golden):
    img = golden["img"]; l, h, w = img.shape
    H = [np.zeros(img.shape, np.float32) for _ in range(6)]
    oracle.orc_hessian3d(golden["F_sig0"], w, h, l, float(golden["sigs"][0]), *H)
    for got, key in zip(H, ("Dzz", "Dyy", "Dyz", "Dxx", "Dxy", "Dxz")):
        assert np.array_equal(got, golden[key]), key


def test_eigen_kat(oracle):
    k = np.load(os.path.join(os.path.dirname(__file__), "golden", "eigen_kat.npz"))
    for A, V, d in zip(k["A"], k["V"], k["d"]):
        v = np.zeros((3, 3)); e = np.zeros(3)
        oracle.orc_eigen3(np.ascontiguousarray(A), v, e)
        assert np.array_equal(v, V) and np.array_equal(e, d)


def test_frangi_matches_reference(oracle, golden):
    J, jmin, jmax, Vx, Vy, Vz = orc.frangi3d(oracle, golden["img"], golden["sigs"], float(golden["zdist"]))
    assert np.array_equal(J, golden["J"])
    assert jmin == golden["Jmin"] and jmax == golden["Jmax"]
    assert np.array_equal(Vx, golden["Vx"]) and np.array_equal(Vy, golden["Vy"]) and np.array_equal(Vz, golden["Vz"])


def test_j8_rule(oracle, golden):
    J8 = orc.j8(oracle, golden["J"], float(golden["Jmin"]), float(golden["Jmax"]))
    assert np.array_equal(J8, golden["J8_restated"])
    # numpy restatement of Advantra_plugin.cpp:2499-2512 (f32 ratio, round half away, clamp)
    r = ((golden["J"] - golden["Jmin"]) / (golden["Jmax"] - golden["Jmin"]) * np.float32(255)).astype(np.float64)
    exp = np.clip(np.where(r > 0, np.floor(r + 0.5), np.ceil(r - 0.5)), 0, 255).astype(np.uint8)
    assert np.array_equal(J8, exp)
    flat = np.zeros(10, np.float32)
    assert orc.j8(oracle, flat, 0.0, 0.0).sum() == 0  # |Jmax-Jmin| <= FLT_MIN branch


def test_seeds_match_reference(oracle, golden):
    s = orc.extract_seeds(oracle, float(golden["tol"]), golden["J8_restated"], golden["Vx"], golden["Vy"], golden["Vz"])
    assert s.shape == golden["seeds"].shape and len(s) > 0
    assert np.array_equal(s, golden["seeds"])


RAGGED = [((33, 21, 9), [2.0], 2.0, 5.0), ((20, 50, 14), [2.0, 3.0], 1.0, 2.0), ((9, 9, 5), [2.0], 2.0, 5.0)]


def ragged_reference(R, img, sigs, zdist, tol, J8):
    img0 = img.copy()
    J, jmin, jmax, Vx, Vy, Vz = orc.frangi3d(R, img, sigs, zdist, prefix="ref")
    return dict(img=img0, J=J, Jmin=np.float32(jmin), Jmax=np.float32(jmax), Vx=Vx, Vy=Vy, Vz=Vz,
                seeds=orc.extract_seeds(R, tol, J8, Vx, Vy, Vz, prefix="ref"))


@pytest.mark.parametrize("shape,sigs,zdist,tol", RAGGED)
def test_live_reference_ragged(oracle, ref, shape, sigs, zdist, tol):
    """ragged / smaller-than-kernel extents against the reference (recorded, and live where built)"""
    w, h, l = shape
    img = synth.synth(w, h, l, seed=3)
    a = orc.frangi3d(oracle, img, sigs, zdist)
    J8 = orc.j8(oracle, a[0], a[1], a[2])
    sa = orc.extract_seeds(oracle, tol, J8, a[3], a[4], a[5])
    for b in references(ref, "ragged_%dx%dx%d" % shape, lambda R: ragged_reference(R, img, sigs, zdist, tol, J8)):
        assert np.array_equal(b["img"], img)
        assert np.array_equal(a[0], b["J"]) and a[1:3] == (float(b["Jmin"]), float(b["Jmax"]))
        for i, k in ((3, "Vx"), (4, "Vy"), (5, "Vz")):
            assert np.array_equal(a[i], b[k])
        assert np.array_equal(sa, b["seeds"])


TOLS = (0.0, 1.0, 5.0, 40.0)


def random_layers():
    """(tol, J8, [Vx, Vy, Vz]) per tolerance: random u8 layers with plateaus, ties, an empty layer and a low-range layer"""
    rs = np.random.RandomState(11)
    for tol in TOLS:
        J8 = (rs.randint(0, 6, (4, 31, 37)) * rs.randint(0, 50, (4, 31, 37))).astype(np.uint8)
        J8[1] = 0  # empty layer: globalMax == globalMin
        J8[2] = np.clip(J8[2], 0, 3)
        V = [rs.randint(0, 256, J8.shape).astype(np.uint8) for _ in range(3)]
        yield tol, J8, V


def random_layers_reference(R):
    out = {}
    for i, (tol, J8, V) in enumerate(random_layers()):
        out.update({f"J8_{i}": J8, f"Vx_{i}": V[0], f"Vy_{i}": V[1], f"Vz_{i}": V[2], f"seeds_{i}": orc.extract_seeds(R, tol, J8, *V, prefix="ref")})
    return out


def test_seeds_random_layers_live(oracle, ref):
    """MaximumFinder on random u8 layers: plateaus, ties and tolerance chains."""
    for b in references(ref, "layers", random_layers_reference):
        for i, (tol, J8, V) in enumerate(random_layers()):
            assert np.array_equal(b[f"J8_{i}"], J8) and all(np.array_equal(b[f"V{c}_{i}"], v) for c, v in zip("xyz", V))
            sa = orc.extract_seeds(oracle, tol, J8, *V)
            assert np.array_equal(sa, b[f"seeds_{i}"], equal_nan=True), tol


def test_glibc_rand_stream(oracle):
    libc = C.CDLL("libc.so.6")
    for seed in (1, 42, 12345, 0):
        libc.srand(seed)
        want = np.array([libc.rand() for _ in range(300)], np.uint32)
        got = np.zeros(300, np.uint32)
        oracle.orc_glibc_rand(seed, 300, got)
        assert np.array_equal(got, want)
    got = np.zeros(4, np.uint32)
    oracle.orc_glibc_rand(42, 4, got)
    assert got.tolist() == [71876166, 708592740, 1483128881, 907283241]  # SURVEY.md section 5 (reference probe)


def test_tracker_table_shapes(oracle):
    """sizes recorded from the reference in SURVEY.md section 8: sz=256 (step 2), ndir=50,
    M_sigma = 845/5625/5625/5625 for sigma 2/4/6/8."""
    T = orc.Tracker(oracle, [2, 4, 6, 8], 2, 20, 5, 3.0, 0.3, zdist=2.0)
    assert T.sz == 256 and T.ndir == 50
    assert [T.model(s)[0].shape[0] for s in range(4)] == [845, 5625, 5625, 5625]
    assert abs(T.table("w0").sum() - 1) < 1e-5 and np.allclose(T.table("w").sum(1), 1, atol=1e-5)
    v = T.table("v")
    assert np.allclose((v * v).sum(1), 1, atol=1e-6)
    assert np.all(np.diff(T.table("w_cws"), axis=1) >= 0)


# ---- soma path: erosion and the u8 Gaussian are pinned on the reference's own frangi.cpp ----
ERODE = [((24, 40, 48), 3), ((5, 7, 9), 4), ((3, 33, 20), 2), ((1, 16, 16), 1)]


def erode_input(shape):
    rng = np.random.default_rng(5)
    l, h, w = shape
    img = rng.integers(0, 256, shape, dtype=np.uint8)
    img[:, h // 4: h // 2, w // 4: w // 2] = 200  # a plateau survives the erosion
    return img


def erode_reference(R, img, rad):
    l, h, w = img.shape
    E = np.zeros_like(img)
    R.ref_imerode_xy(img.copy(), w, h, l, float(rad), E)
    G = E.copy()
    R.ref_imgaussian_u8_xy(G, w, h, l, float(rad))
    return dict(img=img.copy(), eroded=E, blurred=G)


@pytest.mark.parametrize("shape,rad", ERODE)
def test_imerode_imgaussian_u8_vs_reference(oracle, ref, shape, rad):
    l, h, w = shape
    img = erode_input(shape)
    Eo = np.zeros_like(img)
    oracle.orc_imerode_xy(img, w, h, l, float(rad), Eo)
    Go = Eo.copy()
    oracle.orc_imgaussian_u8_xy(Go, w, h, l, float(rad))
    for b in references(ref, "erode_%dx%dx%d_r%d" % (*shape, rad), lambda R: erode_reference(R, img, rad)):
        assert np.array_equal(b["img"], img)
        assert np.array_equal(Eo, b["eroded"])
        assert np.array_equal(Go, b["blurred"]) and Go.max() > 0


# ---- the Gaussian radii the fixtures above leave out (tests/golden/ref_radii.npz: make_golden.py ref_radii) ----
# (sigma, zdist) -> radii (xy, z): (1/6, 1) the smallest, 1 and 1; (0.3, 4) 1 and 1 with z taps of 2.5e-39, below FLT_MIN; (3.5, 3) 11
# and 4; (10, 3) 30 and 10; (20, 1) 60 and 60, the largest sigma a context accepts -- wider than every extent of the stack
GAUSS_RADII = [(1 / 6, 1.0), (0.3, 4.0), (3.5, 3.0), (10.0, 3.0), (20.0, 1.0)]


def gauss_radii_input():
    """random bytes with an empty plane and a band of values 0..3: at (0.3, 4) the empty plane's result is the neighbours' values times
    the outer z taps alone, denormal where it comes from the band"""
    img = np.random.default_rng(7).integers(0, 256, (7, 9, 40), dtype=np.uint8)
    img[:, :, :8] //= 64
    img[3] = 0
    return img


def gauss_radii_reference(R, img, sig, zdist):
    l, h, w = img.shape
    F = np.zeros(img.shape, np.float32)
    R.ref_imgaussian3d(img.copy(), w, h, l, sig, zdist, F)
    return dict(img=img.copy(), F=F)


@pytest.mark.parametrize("sig,zdist", GAUSS_RADII)
def test_imgaussian3d_radii_vs_reference(oracle, ref, sig, zdist):
    img = gauss_radii_input()
    l, h, w = img.shape
    Fo = np.zeros(img.shape, np.float32)
    oracle.orc_imgaussian3d(img, w, h, l, sig, zdist, Fo)
    for b in references(ref, "gauss_s%.4g_z%g" % (sig, zdist), lambda R: gauss_radii_reference(R, img, sig, zdist), REF_RADII):
        assert np.array_equal(b["img"], img)
        assert np.array_equal(Fo, b["F"]) and Fo.max() > 0
    if (sig, zdist) == (0.3, 4.0):
        tiny = np.finfo(np.float32).tiny
        assert ((Fo[3] > 0) & (Fo[3] < tiny)).sum() > 10 and (Fo[3] >= tiny).sum() > 100


# somaradius 1, 6 and 21 (Gaussian radii 3, 18 and 63, erosion windows 3, 13 and 43) on a stack narrower than the widest window, and
# the stacks without contrast: the byte-wise running sum of the u8 Gaussian turns 255 into 246 and 37 into 31
ERODE_RADII = [1, 6, 21]
ERODE_FLAT = [(255, 246), (37, 31)]


def erode_radii_input():
    """a noisy ramp along x, y and z, no voxel below 40: its minimum filter is a ramp again, so the eroded stack keeps a value of its
    own in most voxels under the widest window too"""
    z, y, x = np.meshgrid(np.arange(2), np.arange(33), np.arange(40), indexing="ij")
    return np.clip(40 + 4 * x + 2 * y + 30 * z + np.random.default_rng(6).integers(0, 6, z.shape), 0, 255).astype(np.uint8)


@pytest.mark.parametrize("rad", ERODE_RADII)
def test_imerode_imgaussian_u8_radii_vs_reference(oracle, ref, rad):
    img = erode_radii_input()
    l, h, w = img.shape
    Eo = np.zeros_like(img)
    oracle.orc_imerode_xy(img, w, h, l, float(rad), Eo)
    Go = Eo.copy()
    oracle.orc_imgaussian_u8_xy(Go, w, h, l, float(rad))
    for b in references(ref, "erode_r%d" % rad, lambda R: erode_reference(R, img, rad), REF_RADII):
        assert np.array_equal(b["img"], img)
        assert np.array_equal(Eo, b["eroded"]) and Eo.min() >= 40 and len(np.unique(Eo)) > 30
        assert np.array_equal(Go, b["blurred"]) and Go.max() > 0 and len(np.unique(Go)) > 10


@pytest.mark.parametrize("value,blurred", ERODE_FLAT)
def test_imgaussian_u8_flat_vs_reference(oracle, ref, value, blurred):
    img = np.full((4, 40, 70), value, np.uint8)
    l, h, w = img.shape
    Go = np.zeros_like(img)
    oracle.orc_imerode_xy(img, w, h, l, 2.0, Go)
    assert np.array_equal(Go, img)
    oracle.orc_imgaussian_u8_xy(Go, w, h, l, 2.0)
    assert np.all(Go == blurred)
    for b in references(ref, "flat_%d" % value, lambda R: erode_reference(R, img, 2), REF_RADII):
        assert np.array_equal(b["img"], img) and np.array_equal(b["eroded"], img)
        assert np.array_equal(Go, b["blurred"])


def test_maxentropy_and_conn3d_properties(oracle):
    """maxentropy_th / conn3d are parity-unpinned restatements (toolbox.cpp needs a Vaa3D header): check what the
    published algorithm guarantees -- threshold between two well separated modes, regions = 26-connected components
    numbered in raster order of their first voxel, centroid and mean radius of a ball."""
    rng = np.random.default_rng(2)
    a = np.concatenate([rng.integers(0, 20, 9000), rng.integers(180, 220, 1000)]).astype(np.uint8)
    th = oracle.orc_maxentropy_th(np.ascontiguousarray(a), len(a))
    assert 19 <= th < 180
    hist = np.bincount(a, minlength=256).astype(np.int64)
    assert oracle.orc_maxentropy_hist(hist) == th
    import scipy.ndimage as ndi
    vol = np.zeros((12, 20, 24), np.uint8)
    vol[2:5, 3:6, 4:9] = 255
    vol[5, 6, 9] = 255          # touches the first block by a corner only: same region with diagonal connectivity
    vol[8:11, 12:18, 2:5] = 255
    zz, yy, xx = np.meshgrid(np.arange(12), np.arange(20), np.arange(24), indexing="ij")
    vol[(xx - 17) ** 2 + (yy - 8) ** 2 + (zz - 6) ** 2 <= 9] = 255
    lab = np.zeros(vol.shape, np.int32)
    xc, yc, zc, rc = (np.zeros(16, np.float32) for _ in range(4))
    n = oracle.orc_conn3d(vol, 24, 20, 12, lab.reshape(-1), 1, 0, 1, xc, yc, zc, rc, 16)
    want, nw = ndi.label(vol > 0, structure=np.ones((3, 3, 3)))
    assert n == nw == 3
    first = [np.flatnonzero(lab.reshape(-1) == k)[0] for k in range(1, n + 1)]
    assert first == sorted(first)  # numbered in raster order
    for k in range(1, n + 1):
        m = lab == k
        assert len(np.unique(want[m])) == 1 and (want == want[m][0]).sum() == m.sum()
        assert np.allclose([xc[k - 1], yc[k - 1], zc[k - 1]], [xx[m].mean(), yy[m].mean(), zz[m].mean()], atol=1e-3)
    ball = int(lab[6, 8, 17])
    assert 1.5 < rc[ball - 1] < 3.0  # mean distance to the centre of a radius-3 ball = 3/4 * 3


# ---- 2-D mode: Frangi::frangi2d / hessian2d pinned on the reference's own frangi.cpp ----
F2D = [((1, 40, 48), [2.0]), ((1, 33, 21), [2.0, 3.0]), ((1, 64, 64), [1.0, 2.0, 4.0]), ((1, 7, 9), [2.0])]


def frangi2d_input(shape):
    _, h, w = shape
    return synth.synth(w, h, 9, seed=4)[4:5].copy() if min(h, w) > 16 else np.random.default_rng(3).integers(0, 255, shape, dtype=np.uint8)


def frangi2d_reference(R, img, sigs):
    _, h, w = img.shape
    out = dict(img=img.copy())
    for i, sg in enumerate(sigs):
        D = [np.zeros(img.shape, np.float32) for _ in range(3)]
        R.ref_hessian2d(img.copy(), w, h, sg, *D)
        out.update({f"D{k}_{i}": d for k, d in enumerate(D)})
    J, jmin, jmax, Vx, Vy, Vz = orc.frangi2d(R, img.copy(), sigs, prefix="ref")
    out.update(J=J, Jmin=np.float32(jmin), Jmax=np.float32(jmax), Vx=Vx, Vy=Vy, Vz=Vz)
    return out


@pytest.mark.parametrize("shape,sigs", F2D)
def test_frangi2d_vs_reference(oracle, ref, shape, sigs):
    _, h, w = shape
    img = frangi2d_input(shape)
    for b in references(ref, "f2d_%dx%d_n%d" % (h, w, len(sigs)), lambda R: frangi2d_reference(R, img, sigs)):
        assert np.array_equal(b["img"], img)
        for i, sg in enumerate(sigs):
            a = [np.zeros(shape, np.float32) for _ in range(3)]
            oracle.orc_hessian2d(img, w, h, sg, *a)
            assert all(np.array_equal(a[k], b[f"D{k}_{i}"]) for k in range(3))
        Jo, jmo, jMo, Vxo, Vyo, Vzo = orc.frangi2d(oracle, img, sigs)
        assert np.array_equal(Jo, b["J"]) and jmo == float(b["Jmin"]) and jMo == float(b["Jmax"])
        assert np.array_equal(Vxo, b["Vx"]) and np.array_equal(Vyo, b["Vy"]) and np.array_equal(Vzo, b["Vz"]) and not Vzo.any()
        if min(h, w) > 16:
            assert jMo > 0.05


# the single-slice Gaussian at the radii 24 and 40 (through the Hessian the reference's frangi.cpp exposes; ref_radii.npz)
F2D_RADII = [24, 40]


def hessian2d_radii_reference(R, img, sig):
    _, h, w = img.shape
    D = [np.zeros(img.shape, np.float32) for _ in range(3)]
    R.ref_hessian2d(img.copy(), w, h, sig, *D)
    return dict(img=img.copy(), D0=D[0], D1=D[1], D2=D[2])


@pytest.mark.parametrize("L", F2D_RADII)
def test_hessian2d_radii_vs_reference(oracle, ref, L):
    img = np.random.default_rng(12).integers(0, 256, (1, 9, 70), dtype=np.uint8)
    sig = (L - 0.5) / 3
    a = [np.zeros(img.shape, np.float32) for _ in range(3)]
    oracle.orc_hessian2d(img, 70, 9, sig, *a)
    for b in references(ref, "h2d_L%d" % L, lambda R: hessian2d_radii_reference(R, img, sig), REF_RADII):
        assert np.array_equal(b["img"], img)
        assert all(np.array_equal(a[k], b["D%d" % k]) and np.abs(a[k]).max() > 0 for k in range(3))


# ---- committed fixtures of the reference's 2-D Frangi and soma filters (tests/golden/make_golden.py) ----
def _load(name):
    return dict(np.load(os.path.join(os.path.dirname(__file__), "golden", name + ".npz")))


@pytest.mark.parametrize("name", ["p2d_96x80_s2-3", "p2d_33x21_s2"])
def test_oracle_2d_matches_golden(oracle, name):
    g = _load(name)
    img = g["img"]; _, h, w = img.shape
    D = [np.zeros(img.shape, np.float32) for _ in range(3)]
    oracle.orc_hessian2d(img, w, h, float(g["sigs"][0]), *D)
    for got, key in zip(D, ("Dyy", "Dxy", "Dxx")):
        assert np.array_equal(got, g[key]), key
    J, jmin, jmax, Vx, Vy, Vz = orc.frangi2d(oracle, img, g["sigs"])
    assert np.array_equal(J, g["J"]) and jmin == g["Jmin"] and jmax == g["Jmax"]
    assert np.array_equal(Vx, g["Vx"]) and np.array_equal(Vy, g["Vy"]) and np.array_equal(Vz, g["Vz"])
    J8 = orc.j8(oracle, J, jmin, jmax)
    assert np.array_equal(J8, g["J8_restated"])
    s = orc.extract_seeds(oracle, float(g["tol"]), J8, Vx, Vy, Vz)
    assert np.array_equal(s, g["seeds"], equal_nan=True)


@pytest.mark.parametrize("name", ["soma_64x56x32_r3", "soma_23x20x9_r2"])
def test_oracle_soma_filters_match_golden(oracle, name):
    g = _load(name)
    img = g["img"]; l, h, w = img.shape
    E = np.zeros_like(img)
    oracle.orc_imerode_xy(img, w, h, l, float(g["rad"]), E)
    assert np.array_equal(E, g["eroded"])
    oracle.orc_imgaussian_u8_xy(E, w, h, l, float(g["rad"]))
    assert np.array_equal(E, g["blurred"])
