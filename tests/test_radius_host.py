"""CPU (no GPU needed): the host side of the measured SWC radii (pnr_measure_radii, include/pnr_hip.h) -- the shell table the device
reads against numpy's shells from the f32 distance, the --radius-* flags of advantra_cli, and the radius kernels' compiler report
(no scratch), read the way test_kernel_resources.py reads it."""
import os
import re
import subprocess
import numpy as np
import pytest
import pnr_amd
import radius_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "pnr_amd", "csrc")
CLI = os.path.join(ROOT, "pnr_amd", "host", "advantra_cli")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fhip-fp32-correctly-rounded-divide-sqrt", "-w"]

GRID = [(zd, rmax, False) for zd in (1, 2, 2.5, 4) for rmax in (1, 7, 32, 64)] + [(zd, rmax, True) for zd in (1, 2.5) for rmax in (1, 7, 32, 64)]


@pytest.mark.parametrize("zd,rmax,is2d", GRID, ids=lambda v: str(v))
def test_offset_table_equals_numpy_shells(zd, rmax, is2d):
    """shell sizes and the membership of every shell as a set; raster order (dz, dy, dx) inside a shell; 2-D: dz = 0 only"""
    starts, off = pnr_amd.radius_offsets(zd, rmax, is2d)
    want = radius_ref.shells(zd, rmax, is2d)
    assert len(starts) == rmax + 2 and starts[0] == 0 and starts[-1] == len(off)
    assert np.array_equal(np.diff(starts), [len(s) for s in want])
    for k, s in enumerate(want):
        got = off[starts[k]:starts[k + 1]]
        key = lambda a: np.lexsort((a[:, 0], a[:, 1], a[:, 2]))
        assert np.array_equal(got, got[key(got)]), k          # raster order as it stands
        assert np.array_equal(got, s[key(s)]), k              # the same set
    assert np.array_equal(off[0], [0, 0, 0])
    if is2d:
        assert not off[:, 2].any()


def test_offset_count_of_the_default_table():
    """(zdist 1, rmax 32, 3-D): 137 064 offsets in the shells O_1 .. O_32 around the centre voxel O_0 -- the lattice points of the
    ball of radius 32"""
    starts, off = pnr_amd.radius_offsets(1, 32, False)
    assert len(off) - 1 == 137064 and starts[1] == 1
    r = np.arange(-32, 33)
    assert len(off) == (np.add.outer(np.add.outer(r * r, r * r), r * r) <= 1024).sum()
    L = pnr_amd.lib.load()
    import ctypes as C
    n = C.c_int64()
    for rmax in (0, 65):
        assert L.pnr_radius_offsets(1.0, rmax, 0, None, None, None, None, 0, C.byref(n)) == -1


def test_restatement_closed_forms():
    """the numpy restatement itself on the solids whose answer is known: a solid cylinder dy^2 + (zd dz)^2 <= R^2 at value 200 measured
    on its axis with thr = 100 gives floor(R) for bg_permille 0 and 10; a Gaussian-profile tube of s = 3 with rel_pct = 50 gives 3 on
    the axis and 2 at 1.3 voxels off it"""
    for zd in (1, 2, 4):
        l, h, w = 40 // zd + 9, 41, 30
        z, y, _ = np.meshgrid(np.arange(l), np.arange(h), np.arange(w), indexing="ij")
        for R in (1, 2.5, 3.5, 6):
            V = np.where((y - 20.0) ** 2 + (zd * (z - l // 2.0)) ** 2 <= R * R, 200, 0).astype(np.uint8)
            for bg in (0, 10):
                k, t = radius_ref.measure(V, zd, [[15, 20, l // 2]], thr=100, rel_pct=0, rmax=32, bg_permille=bg)
                assert k[0] == int(R) and t == 100, (zd, R, bg, k)
    z, y, _ = np.meshgrid(np.arange(41), np.arange(41), np.arange(30), indexing="ij")
    V = np.round(200 * np.exp(-((y - 20.0) ** 2 + (z - 20.0) ** 2) / (2 * 3.0 ** 2))).astype(np.uint8)
    k, t = radius_ref.measure(V, 1, [[15, 20, 20], [15, 21.3, 20]], rel_pct=50)
    assert k.tolist() == [3, 2] and t == 0


def run(*args):
    return subprocess.run([CLI, *args], capture_output=True, text=True, timeout=120)


def test_cli_radius_flags():
    """every out-of-range --radius-* value is a usage error that names its flag, before any device call (the test runs without a GPU);
    --help lists the flags"""
    paras = "2 0 5 0.3 3 2 10 20 2 4 1".split()
    bad = [("--radius-max", "0"), ("--radius-max", "65"), ("--radius-max", "x"), ("--radius-threshold", "-2"), ("--radius-threshold", "256"),
           ("--radius-rel", "0"), ("--radius-rel", "101"), ("--radius-rel", "-1"), ("--radius-bg", "-1"), ("--radius-bg", "1000"), ("--radius-bg", "")]
    for flag, val in bad:
        r = run("--measure-radius", flag, val, "-f", "advantra_func", "-i", "missing.tif", "-p", *paras)
        assert r.returncode == 1 and flag in r.stderr and "cannot open" not in r.stderr, (flag, val, r.stderr)
    r = run("--measure-radius", "--radius-threshold", "10", "--radius-rel", "40", "-f", "advantra_func", "-i", "missing.tif", "-p", *paras)
    assert r.returncode == 1 and "--radius-threshold" in r.stderr and "--radius-rel" in r.stderr
    r = run("--radius-max", "8", "-f", "advantra_func", "-i", "missing.tif", "-p", *paras)  # without --measure-radius
    assert r.returncode == 1 and "--measure-radius" in r.stderr
    r = run("--measure-radius", "--radius-nonsense", "1", "-f", "advantra_func", "-i", "missing.tif", "-p", *paras)
    assert r.returncode == 1 and "--radius-nonsense" in r.stderr
    # in-range values pass the parser: the next thing that fails is the missing image
    r = run("--measure-radius", "--radius-threshold", "-1", "--radius-max", "64", "--radius-bg", "999", "-f", "advantra_func", "-i", "missing.tif", "-p", *paras)
    assert r.returncode == 0 and "cannot open" in r.stderr
    h = run("--help")
    assert h.returncode == 0 and "usage of Advantra" in h.stdout
    for flag in ("--measure-radius", "--radius-threshold", "--radius-rel", "--radius-max", "--radius-bg"):
        assert flag in h.stdout, flag


def test_radius_kernels_compile_without_scratch(tmp_path):
    """the compiler's own report (-Rpass-analysis=kernel-resource-usage) for gfx950: radius.hip has exactly one kernel, without scratch and
    light enough for eight waves per SIMD (one wave = one node: occupancy is what hides the gathers)"""
    out = str(tmp_path / "radius.s")
    r = subprocess.run(["/opt/rocm/bin/hipcc", *FLAGS, "-Rpass-analysis=kernel-resource-usage", "-S", "--cuda-device-only", "radius.hip", "-o", out],
                       cwd=SRC, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    usage, name = {}, None
    for ln in r.stderr.splitlines():
        m = re.search(r"remark: [^ ]* *Function Name: (\S+)", ln)
        if m:
            name = m.group(1)
            usage[name] = {}
            continue
        m = re.search(r"remark: [^ ]* *(VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)", ln)
        if m and name:
            usage[name][m.group(1).split(" ")[0]] = int(m.group(2))
    assert len(usage) == 1, list(usage)  # the byte sum behind thr = -1 is volume.hip's (test_volume_resources.py)
    kernels = {frag: [u for k, u in usage.items() if frag in k] for frag in ("rad_measure",)}
    for frag, hit in kernels.items():
        assert len(hit) == 1, (frag, list(usage))
        assert hit[0]["ScratchSize"] == 0, (frag, hit[0])
    assert kernels["rad_measure"][0]["VGPRs"] <= 64 and kernels["rad_measure"][0]["Occupancy"] == 8, kernels["rad_measure"][0]
    assert not re.search(r"^\s+scratch_(load|store)", open(out).read(), re.M)
