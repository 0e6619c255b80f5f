"""CPU: the numpy restatement of pnr_filter_volume's rule (filter_ref.py) against a brute-force triple loop written straight from
include/pnr_hip.h, the property o <= V the rule relies on, and the CLI's handling of --median / --subtract-background before any
GPU is touched."""
import os
import subprocess
import numpy as np
import pytest
import filter_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "pnr_amd", "host", "advantra_cli")
PARAS = "2 0 5 0.3 3 2 20 20 2 4 5".split()


def brute_median(V, mode):
    l, h, w = V.shape
    out = np.zeros_like(V)
    dzs = (-1, 0, 1) if mode == 3 else (0,)
    for z in range(l):
        for y in range(h):
            for x in range(w):
                s = sorted(int(V[min(max(z + dz, 0), l - 1), min(max(y + dy, 0), h - 1), min(max(x + dx, 0), w - 1)])
                           for dz in dzs for dy in (-1, 0, 1) for dx in (-1, 0, 1))
                out[z, y, x] = s[13 if mode == 3 else 4]
    return out


def brute_box(V, radii, fn):
    l, h, w = V.shape
    rz, ry, rx = radii
    out = np.zeros_like(V)
    for z in range(l):
        for y in range(h):
            for x in range(w):
                out[z, y, x] = fn(V[max(z - rz, 0):z + rz + 1, max(y - ry, 0):y + ry + 1, max(x - rx, 0):x + rx + 1])
    return out


def brute_tophat(V, R, zdist):
    rz = 0 if V.shape[0] == 1 else int(np.float32(R) / np.float32(zdist))
    e = brute_box(V, (rz, R, R), np.min)
    o = brute_box(e, (rz, R, R), np.max)
    assert (o <= V).all()
    return V - o


@pytest.mark.parametrize("shape", [(6, 5, 4), (1, 2, 2)], ids=["4x5x6", "2x2x1"])
def test_restatement_against_brute_force(shape):
    rng = np.random.default_rng(3)
    for V in (rng.integers(0, 256, shape, dtype=np.uint8), (rng.integers(0, 2, shape, dtype=np.uint8) * 255).astype(np.uint8),
              rng.integers(100, 103, shape, dtype=np.uint8)):
        for mode in (2, 3):
            assert np.array_equal(filter_ref.median(V, mode), brute_median(V, mode)), (shape, mode)
        if shape[0] == 1:
            assert np.array_equal(filter_ref.median(V, 3), filter_ref.median(V, 2))  # follows from the rule
        for R in (1, 2, 7, 64):
            for zd in (1.0, 2.0, 3.5):
                want = brute_tophat(V, R, zd)
                assert np.array_equal(filter_ref.tophat(V, R, zd), want), (shape, R, zd)
                assert np.array_equal(filter_ref.apply(V, 0, R, zd), want)
        assert np.array_equal(filter_ref.apply(V, 3, 2, 2.0), brute_tophat(brute_median(V, 3), 2, 2.0))
        assert np.array_equal(filter_ref.apply(V, 0, 0, 2.0), V)


def test_box_half_widths():
    assert filter_ref.box(7, 2.0, 10) == (3, 7, 7) and filter_ref.box(7, 3.5, 10) == (2, 7, 7) and filter_ref.box(1, 2.0, 10) == (0, 1, 1)
    assert filter_ref.box(64, 1.0, 10) == (64, 64, 64) and filter_ref.box(64, 1.0, 1) == (0, 64, 64)


def test_opening_never_exceeds_the_volume():
    rng = np.random.default_rng(4)
    for shape in ((7, 19, 23), (1, 30, 31), (12, 3, 2)):
        for V in (rng.integers(0, 256, shape, dtype=np.uint8), (rng.random(shape) < 0.05).astype(np.uint8) * 255):
            for R, zd in ((1, 1.0), (3, 2.0), (9, 3.5), (64, 1.0)):
                o = filter_ref.opening(V, R, zd)
                assert (o <= V).all()
                t = filter_ref.tophat(V, R, zd)
                assert t.dtype == np.uint8 and np.array_equal(t.astype(int), V.astype(int) - o.astype(int))


def _cli(*args):
    if not os.path.exists(CLI):
        subprocess.run(["make", "-s", "-C", os.path.dirname(CLI)], check=True)
    return subprocess.run([CLI, *args], capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("flags,msg", [(("--median", "4"), "--median 2d|3d"), (("--median", "3"), "--median 2d|3d"), (("--median",), "--median 2d|3d"),
                                       (("--subtract-background", "0"), "--subtract-background R"),
                                       (("--subtract-background", "65"), "--subtract-background R"),
                                       (("--subtract-background", "4x"), "--subtract-background R")])
def test_cli_refuses_bad_filter_flags_before_any_gpu_call(tmp_path, flags, msg):
    """status 1 and the flag's usage line; the (valid) stack is never opened: no library message, no SWC"""
    import synth
    raw = str(tmp_path / "s.raw")
    synth.synth(32, 24, 8, seed=1).tofile(raw)
    r = _cli("-d", "32,24,8", *flags, "-f", "advantra_func", "-i", raw, "-p", *PARAS)
    assert r.returncode == 1 and msg in r.stderr, (r.returncode, r.stderr)
    assert "HIP" not in r.stderr and "ADVANTRA" not in r.stdout and not os.path.exists(raw + "_Advantra.swc")


def test_cli_help_names_both_flags():
    r = _cli("--help")
    assert r.returncode == 0 and "--median 2d|3d" in r.stdout and "--subtract-background R" in r.stdout
