"""Every form of the Gaussian stage at every radius its dispatch switches name, and the generic kernels at the radii in between and
up to 60, against the oracle's scalar loop (orc_imgaussian3d / orc_imgaussian2d) -- bit for bit, as the contract says.

frangi.hip picks a kernel per pass from the tap radius L = ceil(3 sigma): the fused x-y kernels (gauss_xy_u8_m / gauss_xy_u8_t), the
templated x pass (gauss_x_u8_t), the templated strided pass (gauss_axis_t) or the generic gauss_x_u8 / gauss_axis.  The radius lists
and the tile sizes are READ FROM THE KERNEL SOURCE here, and the cases are built from them: a radius added to a switch gets its
cases without anyone remembering to.  Which form a case reaches follows from those lists and is checked through the launch count
of the "gauss" timer group (fused x-y: one launch for x and y; pass by pass: two).

Inputs are uniform random bytes, so every voxel and every border carries information; a stack is thin except along the axis under
test.  The extents come from the tile of the form under test: 2, L - 1 (narrower than the halo), one tile exactly and one voxel
less and more, and an interior tile (for the x forms that read whole dwords there: one that takes that path) followed by a ragged
one."""
import os
import re
import numpy as np
import pytest
import orc
import synth
import pnr_amd
from test_gpu_frangi import J_RTOL

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = open(os.path.join(ROOT, "pnr_amd", "csrc", "frangi.hip")).read()


def _switch(name):
    """the radii of a dispatch switch: `PNR_GA(2) PNR_GA(3) ...` (the #define line spells its argument LL)"""
    got = [int(v) for v in re.findall(r"\b%s\((\d+)\)" % name, SRC)]
    assert got, "no radius list found for %s in frangi.hip" % name
    assert len(set(got)) == len(got)
    return got


def _constants(names):
    got = {}
    for line in re.findall(r"^constexpr int ([^;]*);", SRC, re.M):
        got.update({k: int(v) for k, v in re.findall(r"\b(\w+) = (\d+)\s*(?=,|$)", line)})
    assert all(k in got for k in names), [k for k in names if k not in got]
    return [got[k] for k in names]


GX, GXM, GXY, GA = _switch("PNR_GX"), _switch("PNR_GXM"), _switch("PNR_GXY"), _switch("PNR_GA")
GX_BLOCK, GXT_W, GXT_H, TA, TAT, GXY_TY, MAX_L = _constants(["GX_BLOCK", "GXT_W", "GXT_H", "TA", "TAT", "GXY_TY", "MAX_L"])
FUSED_W = 64  # columns of a fused x-y tile (a wave-row)


def generic(radii, *lists):
    """those of `radii` that no switch in `lists` names: the ones the generic kernel takes"""
    out = [L for L in radii if not any(L in s for s in lists) and L <= MAX_L]
    assert out and max(out) >= 40, "a generic case at L >= 40 is required"
    return out


def xy_form(L, march):
    """the kernel the x pass of radius L runs in (gaussian3d's dispatch order)"""
    if march and L in GXM:
        return "gauss_xy_u8_m"
    if L in GXY:
        return "gauss_xy_u8_t"
    return "gauss_x_u8_t" if L in GX else "gauss_x_u8"


def axis_form(L):
    return "gauss_axis_t" if L in GA else "gauss_axis"


def radii(sig, zdist):
    """(Lxy, Lz) as pnr::gaussian_taps computes them: f32 product, f32 ceil"""
    s, zd = np.float32(sig), np.float32(zdist)
    return int(np.ceil(np.float32(3) * s)), int(np.ceil(np.float32(3) * np.float32(s / zd)))


def sigma_for(L):
    return (L - 0.5) / 3


def drive_z(Lz):
    """(sigma, zdist) with ceil(3 sigma / zdist) = Lz and, where MAX_L allows it, another radius in the plane (so that a pass that
    took the other axis' taps cannot pass)"""
    for zdist in (4.0, 1.5, 1.0):
        sig = sigma_for(Lz) * zdist
        lxy, lz = radii(sig, zdist)
        if lz == Lz and lxy <= MAX_L and (lxy != Lz or zdist == 1.0):
            return sig, zdist
    raise AssertionError(Lz)


@pytest.fixture(scope="module")
def ctxs():
    """one Context per zdist, shared by the cases of this file (a Context builds the tracker's tables when it is made)"""
    made = {}

    def get(zdist):
        if zdist not in made:
            made[zdist] = pnr_amd.Context(pnr_amd.make_params(sigmas=[2.0], zdist=zdist, np_=20, ni=5), 0)
            made[zdist].set_profiling(True)
        return made[zdist]
    yield get
    for c in made.values():
        c.close()


def random_stack(shape, seed=0):
    return np.random.default_rng([seed, *shape]).integers(0, 256, shape, dtype=np.uint8)


def check(oracle, ctxs, img, sig, zdist, march, want_radii):
    """F of the device == F of the oracle on `img`, at the intended radii, through the expected number of launches"""
    l, h, w = img.shape
    assert radii(sig, zdist) == want_radii, (radii(sig, zdist), want_radii)
    Lxy = want_radii[0]
    want = np.empty(img.shape, np.float32)
    if l == 1:
        oracle.orc_imgaussian2d(img, w, h, sig, want)
    else:
        oracle.orc_imgaussian3d(img, w, h, l, sig, zdist, want)
    c = ctxs(zdist)
    c.set_option("gauss_march", march)
    c.set_volume(img)
    c.reset_kernel_ms()
    F = c.gaussian(sig)
    launches = c.kernel_ms("gauss")[1]
    assert F.max() > 0
    bad = np.flatnonzero(F.reshape(-1) != want.reshape(-1))
    assert len(bad) == 0, "%s L=%s march=%d: %d voxels differ, first at (z, y, x) = %s" % (
        img.shape, want_radii, march, len(bad), np.unravel_index(bad[0], img.shape))
    assert np.array_equal(F, want)  # (NaN would pass the line above)
    fused = xy_form(Lxy, march).startswith("gauss_xy")
    assert launches == (1 if l == 1 else 2) + (0 if fused else 1), (launches, xy_form(Lxy, march))


def extents(L, tile, last):
    return sorted({n for n in (2, L - 1, tile - 1, tile, tile + 1, last) if n >= 2})  # (a volume is at least 2 x 2 x 1)


# ---------------------------------------------------------------- x axis
X_GENERIC = generic((1, 2, 7, 10, 25, 40, 60), GX, GXM, GXY)
X_CASES = ([(L, m) for L in sorted(set(GXM) | set(GXY)) for m in (1, 0)] +
           [(L, 1) for L in GX if L not in GXM and L not in GXY] + [(L, 1) for L in X_GENERIC])


def x_widths(L, form):
    if form == "gauss_x_u8":  # an interior tile whose left halo is data, a ragged third whose right clamp lies in a later tile
        return extents(L, GX_BLOCK, 2 * GX_BLOCK + L + 3)
    tw = GXT_W if form == "gauss_x_u8_t" else FUSED_W
    x0 = -(-L // tw) * tw  # the first tile with x0 - L >= 0; x0 + tw + L + 4 <= w lets it read whole dwords
    return extents(L, tw, x0 + tw + L + 4 + 3)


@pytest.mark.parametrize("L,march", X_CASES, ids=["L%d-march%d" % c for c in X_CASES])
def test_x_axis(oracle, ctxs, L, march):
    """(l, h) = (3, 5), the width from the tile of the form the radius takes"""
    form = xy_form(L, march)
    for w in x_widths(L, form):
        check(oracle, ctxs, random_stack((3, 5, w)), sigma_for(L), 1.0, march, (L, L))
    if form == "gauss_x_u8":
        assert max(x_widths(L, form)) > 2 * GX_BLOCK
    if form == "gauss_x_u8_t":  # a row tile of one row: h l = GXT_H + 1
        rows = GXT_H + 1
        l = next(d for d in range(2, rows) if rows % d == 0)
        check(oracle, ctxs, random_stack((l, rows // l, max(x_widths(L, form)))), sigma_for(L), 1.0, march, (L, L))


# ---------------------------------------------------------------- y and z axes
A_GENERIC = generic((1, 4, 7, 10, 25, 40, 60), GA)
Y_CASES = [(L, m) for L in GA + A_GENERIC for m in ((1, 0) if L in GXM or L in GXY else (1,))]
Z_CASES = sorted(set(GA + A_GENERIC + [1, 24]))


def axis_extents(L, form):
    t = TAT if form != "gauss_axis" else TA
    return extents(L, t, 2 * t + 7)


@pytest.mark.parametrize("L,march", Y_CASES, ids=["L%d-march%d" % c for c in Y_CASES])
def test_y_axis(oracle, ctxs, L, march):
    """(l, w) = (3, 65): one lane of the second x tile is active.  A radius of the fused lists has its y pass inside the fused
    kernel (tiles / chunks of GXY_TY rows), every other one in gauss_axis_t or gauss_axis"""
    assert GXY_TY == TAT
    form = xy_form(L, march) if xy_form(L, march).startswith("gauss_xy") else axis_form(L)
    for h in axis_extents(L, form):
        check(oracle, ctxs, random_stack((3, h, 65)), sigma_for(L), 1.0, march, (L, L))


@pytest.mark.parametrize("Lz", Z_CASES, ids=["Lz%d" % L for L in Z_CASES])
def test_z_axis(oracle, ctxs, Lz):
    """(h, w) = (3, 65); the z radius through zdist"""
    sig, zdist = drive_z(Lz)
    for l in axis_extents(Lz, axis_form(Lz)):
        check(oracle, ctxs, random_stack((l, 3, 65)), sig, zdist, 1, (radii(sig, zdist)[0], Lz))


def test_generic_kernels_ran_long_and_over_two_tiles():
    """what the parametrisation above holds for the generic kernels: L >= 40 over more than two tiles of their own size, per axis"""
    assert any(L >= 40 and xy_form(L, m) == "gauss_x_u8" and max(x_widths(L, "gauss_x_u8")) > 2 * GX_BLOCK for L, m in X_CASES)
    assert any(L >= 40 and axis_form(L) == "gauss_axis" and max(axis_extents(L, "gauss_axis")) > 2 * TA for L, _ in Y_CASES)
    assert any(L >= 40 and axis_form(L) == "gauss_axis" and max(axis_extents(L, "gauss_axis")) > 2 * TA for L in Z_CASES)
    for lst in (GX, GXM, GXY):
        assert all((L, 1) in X_CASES for L in lst)
    assert all((L, 1) in Y_CASES and L in Z_CASES for L in GA)


# ---------------------------------------------------------------- single slice
@pytest.mark.parametrize("L", [1, 6, 9, 24, 40])
@pytest.mark.parametrize("w,h", [(70, 41), (300, 9)])
def test_single_slice(oracle, ctxs, w, h, L):
    """l = 1: no z pass (frangi.cpp:576-645); y writes the result"""
    for march in ((1, 0) if L in GXM or L in GXY else (1,)):
        check(oracle, ctxs, random_stack((1, h, w)), sigma_for(L), 2.0, march, (L, radii(sigma_for(L), 2.0)[1]))


# ---------------------------------------------------------------- denormal taps
def test_denormal_z_taps(oracle, ctxs):
    """sigma 0.3, zdist 4: Lz = 1 and the outer z taps are exp(-1 / (2 0.075^2)) = 2.5e-39, below FLT_MIN.  The reference multiplies
    by them in IEEE arithmetic.  Where the middle tap meets data the product is absorbed; in an empty plane between two planes of
    data it IS the result, so the stack has such planes, and a band of small values (their products with the tap are denormal
    themselves)"""
    sig, zdist = 0.3, 4.0
    tap = np.float32(np.exp(-1.0 / (2 * float(np.float32(sig) / np.float32(zdist)) ** 2)))
    assert 0 < tap < np.finfo(np.float32).tiny
    img = random_stack((7, 9, 40), seed=3)
    img[:, :, :12] //= 64  # 0..3
    img[2] = 0
    img[5] = 0
    want = np.empty(img.shape, np.float32)
    oracle.orc_imgaussian3d(img, 40, 9, 7, sig, zdist, want)
    tiny = np.finfo(np.float32).tiny
    assert ((want[2] > 0) & (want[2] < tiny)).sum() > 20 and ((want[5] >= tiny) & (want[5] < 1e-30)).sum() > 20
    check(oracle, ctxs, img, sig, zdist, 1, (1, 1))


# ---------------------------------------------------------------- the whole Frangi on radii no default produces
def test_frangi_on_unusual_radii(oracle):
    """sigmas 1, 3.5, 10 at zdist 3: xy radii 3, 11, 30 and z radii 1, 4, 10 -- generic x and y passes at every scale, generic z at
    all three -- under the Hessian, the solver, the maximum over the scales and J8.  Tubes along x and along z (two synthetic stacks,
    one transposed) give a response in every plane"""
    w, h, l = 270, 24, 20
    sigs, zdist = [1.0, 3.5, 10.0], 3.0
    assert [radii(s, zdist) for s in sigs] == [(3, 1), (11, 4), (30, 10)]
    img = np.ascontiguousarray(np.maximum(synth.synth(w, h, l, seed=11), synth.synth(l, h, w, seed=12).transpose(2, 1, 0)))
    J, jmin, jmax, Vx, Vy, Vz = orc.frangi3d(oracle, img, sigs, zdist)
    assert all((J[z] > 0).any() for z in range(l))
    J8 = orc.j8(oracle, J, jmin, jmax)
    c = pnr_amd.Context(pnr_amd.make_params(sigmas=sigs, zdist=zdist), 0)
    c.set_volume(img)
    gmin, gmax = c.frangi()
    assert np.array_equal(c.get_frangi(J=False, J8=True, V=False)["J8"], J8)  # the pruned run's J8
    g = c.get_frangi()
    assert np.array_equal(g["Vx"], Vx) and np.array_equal(g["Vy"], Vy) and np.array_equal(g["Vz"], Vz)
    assert np.allclose(g["J"], J, rtol=J_RTOL, atol=0)
    assert gmin == jmin and abs(gmax - jmax) <= J_RTOL * jmax
    assert np.array_equal(g["J8"], J8)
    c.close()
