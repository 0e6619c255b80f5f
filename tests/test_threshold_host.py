"""CPU: the threshold rules of include/pnr_hip.h (pnr_threshold_from_hist, pure host) against their numpy restatement
(threshold_ref.py) on the histograms where the rules can go wrong, every argument error with its text, the restatement of the local
threshold against its own triple loop, and the methods on the synthetic test stack: they are not one number under three names."""
import ctypes as C
import numpy as np
import pytest
import synth
import pnr_amd
from pnr_amd import lib
import threshold_ref as ref

LOS = (0, 1, 17, 255)
PPMS = (1, 10000, 999999)


def _h(**bins):
    H = np.zeros(256, np.uint64)
    for k, v in bins.items():
        H[int(k[1:])] = v
    return H


def histograms():
    rng = np.random.default_rng(5)
    out = {}
    for k in range(6):
        out[f"random{k}"] = rng.integers(0, 10**(k + 1), 256).astype(np.uint64)
    sparse = rng.integers(0, 1000, 256).astype(np.uint64)
    sparse[rng.random(256) < 0.7] = 0
    out["sparse"] = sparse
    out["empty"] = _h()
    for b in (0, 1, 16, 17, 18, 254, 255):
        out[f"one_bin_{b}"] = _h(**{f"b{b}": 9})
    out["two_bins"] = _h(b3=10, b200=5)
    out["two_bins_adjacent"] = _h(b17=4, b18=4)
    out["two_bins_ends"] = _h(b0=1, b255=1)
    out["below_lo_only"] = _h(b0=50, b5=7, b16=2)
    out["equal_peaks"] = _h(b20=100, b40=100, b60=100, b90=3)
    flat = np.full(256, 7, np.uint64)
    out["flat"] = flat
    stretch = np.zeros(256, np.uint64)
    stretch[10] = 1000
    stretch[11:200] = 5  # a flat stretch below the chord: g falls with b, the first b wins
    stretch[200] = 5
    out["flat_stretch"] = stretch
    steps = np.zeros(256, np.uint64)
    steps[30:60], steps[60:120], steps[120:130] = 50, 10, 50  # ties of Otsu's score cannot be built by hand; ties of g can
    out["steps"] = steps
    big = np.zeros(256, np.uint64)
    big[2], big[100], big[255] = 2**33, 2**33 + 1, 2**33
    out["bins_2_33"] = big
    big2 = (rng.integers(0, 2**33, 256).astype(np.uint64) + np.uint64(2**33))
    out["all_bins_above_2_33"] = big2
    out["top_bin_heavy"] = _h(b0=10, b255=10**6)  # H[255] > k for every share
    return out


HISTS = histograms()


@pytest.mark.parametrize("name", list(HISTS))
def test_methods_match_the_restatement(name):
    H = HISTS[name]
    for lo in LOS:
        for method in ("mean", "otsu", "triangle"):
            assert pnr_amd.threshold_from_hist(H, method, lo) == ref.from_hist(H, method, lo), (name, method, lo)
        for ppm in PPMS:
            assert pnr_amd.threshold_from_hist(H, "top", lo, ppm) == ref.from_hist(H, "top", lo, ppm), (name, lo, ppm)


def test_the_edge_cases_are_the_ones_meant():
    assert ref.from_hist(HISTS["below_lo_only"], "otsu", 17)["n_counted"] == 0 and ref.from_hist(HISTS["below_lo_only"], "otsu", 17)["thr"] == 255
    assert ref.from_hist(HISTS["top_bin_heavy"], "top", 0, 10000)["thr"] == 255  # H[255] > k: no t has few enough voxels at or above it
    assert ref.from_hist(HISTS["equal_peaks"], "triangle", 0)["peak"] == 20
    assert ref.from_hist(HISTS["one_bin_0"], "otsu", 0)["thr"] == 1  # zero is never foreground
    assert ref.from_hist(HISTS["one_bin_18"], "otsu", 0)["thr"] == 18
    assert ref.from_hist(HISTS["flat_stretch"], "triangle", 0)["thr"] == 12


def test_mean_is_the_rule_of_minus_one():
    rng = np.random.default_rng(6)
    for k in range(20):
        V = (rng.integers(0, 256, 5000) * rng.random()).astype(np.uint8)
        if k == 0:
            V[:] = 0
        got = pnr_amd.threshold_from_hist(ref.histogram(V), "mean", 0)
        assert got["thr"] == max(1, int(V.sum(dtype=np.int64)) // V.size)
        assert got["n_fg"] == int((V >= got["thr"]).sum()) and got["n_vox"] == V.size


def test_maxentropy_is_the_oracles(oracle):
    fn = oracle.orc_maxentropy_hist
    for name, H in HISTS.items():
        if int(H.max()) >= 2**31 or int(H.sum()) == 0:
            continue
        assert pnr_amd.threshold_from_hist(H, "maxentropy") == ref.from_hist(H, "maxentropy", maxentropy=fn), name
    img = synth.synth(48, 40, 24, seed=1, zdist=2.0)
    H = ref.histogram(img)
    assert pnr_amd.threshold_from_hist(H, "maxentropy")["thr"] == max(1, int(fn(H.astype(np.int64))))


def test_maxentropy_at_the_width_of_the_references_int(oracle):
    """the rule reads a bin as `int`: 2^31 - 1 is the largest count it reads whole -- accepted, and the oracle's threshold -- and 2^31
    is refused, in bin 0 (a dark stack above 2^31 voxels) as anywhere else.  pnr_soma asks the same function (test_gpu_soma.py)"""
    fn = oracle.orc_maxentropy_hist
    rng = np.random.default_rng(7)
    tubes = np.zeros(256, np.uint64)
    tubes[1:220] = rng.integers(0, 4000, 219)
    for b in (0, 100):
        H = tubes.copy()
        H[b] = 2**31 - 1
        got = pnr_amd.threshold_from_hist(H, "maxentropy")
        assert got == ref.from_hist(H, "maxentropy", maxentropy=fn) and got["thr"] == max(1, int(fn(H.astype(np.int64)))) and got["n_vox"] == int(H.sum()), b
        H[b] = 2**31
        _fails("pnr_threshold_from_hist: maxentropy needs every bin below 2^31, bin %d holds 2147483648" % b, H, "maxentropy")
    H = tubes.copy()
    H[0] = 2248146944 - int(tubes.sum())  # the bin 0 of a sparse 2048 x 2048 x 536 stack
    _fails("pnr_threshold_from_hist: maxentropy needs every bin below 2^31, bin 0 holds %d" % int(H[0]), H, "maxentropy")


def _fails(text, *args):
    with pytest.raises(pnr_amd.PnrError) as e:
        pnr_amd.threshold_from_hist(*args)
    assert text in str(e.value) and "error -1" in str(e.value), str(e.value)


def test_argument_errors_and_their_texts():
    H = HISTS["two_bins"]
    who = "pnr_threshold_from_hist: "
    _fails(who + "method = 5 outside [0, 4]", H, 5)
    _fails(who + "method = -1 outside [0, 4]", H, -1)
    _fails(who + "lo = 256 outside [0, 255]", H, "otsu", 256)
    _fails(who + "lo = -1 outside [0, 255]", H, "mean", -1)
    _fails(who + "top_ppm = 0 outside [1, 999999]", H, "top", 0)
    _fails(who + "top_ppm = 1000000 outside [1, 999999]", H, "top", 0, 1000000)
    _fails(who + "top_ppm = 7, not 0 (only method 3 takes a share)", H, "otsu", 0, 7)
    _fails(who + "maxentropy needs lo = 0, not 1", H, "maxentropy", 1)
    _fails(who + "maxentropy needs every bin below 2^31, bin 100 holds 2147483648", _h(b3=1, b100=2**31), "maxentropy")
    _fails(who + "more than 2^45 - 1 voxels (bin 9 holds 35184372088832)", _h(b9=2**45), "mean")
    _fails(who + "more than 2^45 - 1 voxels (bin 10 holds 1)", _h(b9=2**45 - 1, b10=1), "mean")
    L = lib.load()
    o, info = lib.ThresholdOpts(1, 0, 0, 0), lib.ThresholdInfo()
    for a in ((None, C.byref(o), C.byref(info)), (H.ctypes.data, None, C.byref(info)), (H.ctypes.data, C.byref(o), None)):
        assert L.pnr_threshold_from_hist(*a) == -1 and L.pnr_last_error() == b"null argument"
    with pytest.raises(ValueError):
        pnr_amd.threshold_from_hist(H, "isodata")
    with pytest.raises(ValueError):
        pnr_amd.threshold_from_hist(H[:100], "otsu")


def test_threshold_words():
    assert pnr_amd.parse_threshold("otsu") == ("otsu", 0, None)
    assert pnr_amd.parse_threshold("triangle:1") == ("triangle", 1, None)
    assert pnr_amd.parse_threshold("top1.5") == ("top", 0, 15000)
    assert pnr_amd.parse_threshold("top0.25:17") == ("top", 17, 2500)
    for bad in ("top", "otsu:x", "isodata", "topx", ""):
        with pytest.raises(ValueError):
            pnr_amd.parse_threshold(bad)


@pytest.mark.parametrize("shape,r,zd", [((1, 1, 1), 1, 1.0), ((1, 5, 6), 2, 2.0), ((5, 6, 7), 1, 1.0), ((5, 6, 7), 3, 2.0), ((4, 3, 7), 64, 3.7), ((5, 6, 7), 2, 3.7)])
def test_summed_table_equals_the_triple_loop(shape, r, zd):
    rng = np.random.default_rng(sum(shape) + r)
    V = rng.integers(0, 256, shape, dtype=np.uint8)
    V[rng.random(shape) < 0.3] = 0
    for offset, scale, floor, binary in ((0, 256, 1, False), (-20, 320, 1, True), (20, 0, 40, False), (0, 4096, 1, False), (5, 200, 40, True)):
        out, info = ref.local(V, r, zd, offset, scale, floor, binary)
        assert np.array_equal(out, ref.local_loops(V, r, zd, offset, scale, floor, binary)), (offset, scale, floor, binary)
        assert info["n_kept"] == int((out > 0).sum()) and info["sum_out"] == int(out.sum(dtype=np.int64))


def test_methods_are_not_degenerate_on_the_synthetic_stack():
    img = synth.synth(48, 40, 24, seed=1, zdist=2.0)
    H = ref.histogram(img)
    got = {m: pnr_amd.threshold_from_hist(H, m, 0, ppm) for m, ppm in (("mean", None), ("otsu", None), ("top", 10000))}
    for m, ppm in (("mean", None), ("otsu", None), ("top", 10000)):
        assert got[m] == ref.from_hist(H, m, 0, ppm)
    assert len({g["thr"] for g in got.values()}) == 3, got
    assert 2 * got["otsu"]["n_fg"] < got["mean"]["n_fg"], got
