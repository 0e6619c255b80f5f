"""16-bit and multi-channel stacks windowed to 8 bits on the GPU (pnr_set_volume_u16[_device], pnr_get_volume): the exact rule of
include/pnr_hip.h replicated in numpy, the window from the stack against np.partition, channels, the pipeline and the CLI on the
mapped bytes."""
import ctypes as C
import os
import subprocess
import numpy as np
import pytest
import synth
import pnr_amd
from pnr_amd import lib
from test_stack_formats import write_tiff

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "pnr_amd", "host", "advantra_cli")


def np_map(x, lo, hi):
    """the rule: (510 a + d) div 2d, a = clamp(v, lo, hi) - lo, d = hi - lo; a constant window: 255 above lo"""
    x = np.asarray(x).astype(np.int64)
    if hi == lo:
        return np.where(x > lo, 255, 0).astype(np.uint8)
    a = np.clip(x, lo, hi) - lo
    d = hi - lo
    return ((510 * a + d) // (2 * d)).astype(np.uint8)


def ranks(n, ppm_lo, ppm_hi):
    return n * ppm_lo // 10**6, n - 1 - n * ppm_hi // 10**6


@pytest.fixture(scope="module")
def ctx():
    c = pnr_amd.Context(pnr_amd.make_params(sigmas=(2, 3)), 0)
    yield c
    c.close()


def test_mapping_exhaustive(ctx):
    """every u16 value through ~40 fixed windows (d = 1, 2, 255, 256, 65535, lo = 0, hi = 65535, ...), the [min, max] default and a
    saturated window: every byte equals the numpy rule"""
    x = np.arange(65536, dtype=np.uint16)
    np.random.default_rng(0).shuffle(x)
    x = x.reshape(16, 64, 64)
    rng = np.random.default_rng(1)
    wins = [(0, 1), (0, 2), (0, 255), (0, 256), (0, 65535), (65534, 65535), (65533, 65535), (65280, 65535), (65279, 65535), (100, 101),
            (100, 102), (1000, 1255), (1000, 1256), (0, 4095), (0, 4096), (0, 1000), (12345, 65535), (1, 65535), (0, 65534), (32767, 32768),
            (255, 256), (256, 512), (3, 7), (0, 3), (9, 65530)]
    while len(wins) < 40:
        lo, hi = sorted(rng.integers(0, 65536, 2).tolist())
        if lo < hi:
            wins.append((lo, hi))
    for lo, hi in wins:
        ctx.set_volume(x, window=(lo, hi))
        assert ctx.window == (lo, hi)
        got = ctx.get_volume()
        assert np.array_equal(got, np_map(x, lo, hi)), (lo, hi, np.flatnonzero(got != np_map(x, lo, hi))[:5])
    ctx.set_volume(x)
    assert ctx.window == (0, 65535) and np.array_equal(ctx.get_volume(), np_map(x, 0, 65535))
    ctx.set_volume(x, window={"saturate": (1.5, 0.35)})
    k_lo, k_hi = ranks(x.size, 15000, 3500)
    assert ctx.window == (k_lo, k_hi) and np.array_equal(ctx.get_volume(), np_map(x, k_lo, k_hi))


def distributions(shape, seed):
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape))
    out = {
        "uniform": rng.integers(0, 65536, n),
        "dark12": np.minimum(100 + rng.exponential(60, n) + (rng.random(n) < 0.02) * rng.integers(0, 4000, n), 4095),
        "constant": np.full(n, 777),
        "two": np.where(rng.random(n) < 0.3, 5000, 60000),
        "onebin": 0x1200 + rng.integers(0, 256, n),
        "extremes": np.where(rng.random(n) < 0.5, 0, 65535),
    }
    return {k: v.astype(np.uint16).reshape(shape) for k, v in out.items()}


PPM = [(0, 0), (0, 3500), (100, 100), (0, 999999)]


@pytest.mark.parametrize("shape", [(1, 2, 2), (7, 5, 3), (33, 129, 257), (40, 1000, 1000)], ids=lambda s: "x".join(map(str, s[::-1])))
def test_window_from_the_stack(ctx, shape):
    """lo_out / hi_out = np.partition at k_lo / k_hi and the bytes of the rule, for six distributions and four saturation pairs"""
    for name, x in distributions(shape, sum(shape)).items():
        flat = x.ravel()
        ks = sorted({k for a, b in PPM for k in ranks(flat.size, a, b)})
        part = np.partition(flat, ks)
        for a, b in PPM:
            k_lo, k_hi = ranks(flat.size, a, b)
            want = (int(part[k_lo]), int(part[k_hi]))
            ctx.set_volume(x, window={"saturate": (a / 1e4, b / 1e4)})
            assert ctx.window == want, (name, a, b, ctx.window, want)
            assert np.array_equal(ctx.get_volume(), np_map(x, *want)), (name, a, b)


def test_smallest_stack_is_the_contract_minimum(ctx):
    """1 x 1 x 1 is below the context's 2 x 2 x 1 minimum, as for 8-bit volumes: PNR_E_ARG"""
    with pytest.raises(lib.PnrError, match="at least 2x2x1"):
        ctx.set_volume(np.zeros((1, 1, 1), np.uint16))


def test_channels_host_and_device(ctx):
    """nchan 2..4, every channel, from host memory and from a torch tensor (also one that starts 2 bytes past an alignment
    boundary): the bytes of that channel alone"""
    import torch
    rng = np.random.default_rng(3)
    shape = (9, 37, 41)
    for nchan in (2, 3, 4):
        x = (rng.integers(0, 4096, shape + (nchan,)) * (np.arange(nchan) + 1)).astype(np.uint16)
        dev = torch.from_numpy(x.view(np.int16)).cuda()
        for ch in range(nchan):
            for win in (None, (50, 3000), {"saturate": (0.1, 0.35)}):
                ctx.set_volume(x, channel=ch, window=win)
                w_host, v_host = ctx.window, ctx.get_volume()
                ctx.set_volume(np.ascontiguousarray(x[..., ch]), window=win)
                assert ctx.window == w_host and np.array_equal(ctx.get_volume(), v_host)
                assert np.array_equal(v_host, np_map(x[..., ch], *w_host))
                torch.cuda.synchronize()
                ctx.set_volume_device(dev.data_ptr(), shape, dtype=np.uint16, nchan=nchan, channel=ch, window=win)
                assert ctx.window == w_host and np.array_equal(ctx.get_volume(), v_host), (nchan, ch, win)
    # one channel from a device pointer that is only 2-byte aligned: the vector loads start after a peeled head
    x = rng.integers(0, 65536, (5, 33, 29), dtype=np.uint16)
    flat = torch.from_numpy(np.concatenate([np.zeros(1, np.uint16), x.ravel()]).view(np.int16)).cuda()
    for win in (None, (1000, 50000), {"saturate": (0, 0.35)}):
        torch.cuda.synchronize()
        ctx.set_volume_device(flat.data_ptr() + 2, x.shape, dtype=np.uint16, window=win)
        ctx.set_volume(x, window=win)
        want = ctx.get_volume()
        ctx.set_volume_device(flat.data_ptr() + 2, x.shape, dtype=np.uint16, window=win)
        assert np.array_equal(ctx.get_volume(), want) and np.array_equal(want, np_map(x, *ctx.window))


def test_errors_and_timer():
    """PNR_E_ARG keeps the previous volume; a failed allocation leaves no volume; the "volume" kernel timer counts launches"""
    L = lib.load()
    c = pnr_amd.Context(pnr_amd.make_params(sigmas=(2,)), 0)
    x = np.random.default_rng(4).integers(0, 4096, (4, 16, 16, 2), dtype=np.uint16)
    c.set_volume(x, channel=1)
    before = c.get_volume()
    lo, hi = C.c_int32(), C.c_int32()

    def call(nchan, channel, win):
        w = lib.make_window(win)
        return L.pnr_set_volume_u16(c.h, x.ctypes.data, 16, 16, 4, nchan, channel, C.byref(w) if w is not None else None, C.byref(lo), C.byref(hi))

    bad = [(0, 0, None), (2, 2, None), (2, -1, None), (2, 0, (9, 9)), (2, 0, (-2, 5)), (2, 0, (0, 65536)), (2, 0, {"saturate": (50, 50)}),
           (2, 0, {"saturate": (-1, 0)})]
    for nchan, channel, win in bad:
        assert call(nchan, channel, win) == -1, (nchan, channel, win, L.pnr_last_error())
        assert np.array_equal(c.get_volume(), before)
    assert L.pnr_set_volume_u16(c.h, None, 16, 16, 4, 1, 0, None, None, None) == -1
    assert L.pnr_get_volume(c.h, None) == -1
    # a stack no device can hold: PNR_E_NOMEM before any sample is read, then no volume (PNR_E_STATE)
    import torch
    t = torch.zeros(64, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    assert L.pnr_set_volume_u16_device(c.h, t.data_ptr(), 1 << 20, 1 << 10, 1 << 20, 1, 0, None, None, None) == -5, L.pnr_last_error()
    buf = np.zeros(16, np.uint8)
    assert L.pnr_get_volume(c.h, buf.ctypes.data) == -4
    c.set_profiling(True)
    for win, n in ((None, 2), ({"saturate": (0, 0.35)}, 5), ((10, 4000), 1)):
        c.reset_kernel_ms()
        c.set_volume(x, channel=0, window=win)
        ms, launches = c.kernel_ms("volume")
        assert launches == n and ms > 0, (win, launches, ms)
    c.reset_kernel_ms()
    c.set_volume(x[..., 0].astype(np.uint8))
    assert c.kernel_ms("volume")[1] == 0  # 8-bit input: no windowing
    c.close()


def deep_stack(img8, seed):
    """a 12-bit stack whose content is img8's: 15 * img8 + noise below one 8-bit step, on a dark offset"""
    rng = np.random.default_rng(seed)
    return (img8.astype(np.uint16) * 15 + 40 + rng.integers(0, 15, img8.shape)).astype(np.uint16)


@pytest.mark.parametrize("case", ["3d", "soma", "slice"])
def test_pipeline_on_u16_equals_pipeline_on_mapped_u8(case):
    """run_pipeline on the 12-bit stack gives the seeds, nodes, links and tree of run_pipeline on the numpy-mapped 8-bit stack"""
    if case == "3d":
        img8, kw = synth.synth(64, 56, 32, seed=2), dict(ni=40, np_=50, vol=5)
    elif case == "soma":
        img8, kw = synth.add_somas(synth.synth(64, 56, 32, seed=2), ((20, 28, 16, 6), (48, 20, 14, 5))), dict(somaradius=3, ni=25, np_=40)
    else:
        img8, kw = np.ascontiguousarray(synth.synth(96, 80, 9, seed=4).max(0, keepdims=True)), dict(ni=25, np_=40)
    x = deep_stack(img8, 5)
    win = {"saturate": (0, 0.35)}
    p = pnr_amd.make_params(sigmas=[2, 3], tolerance=5, znccth=0.3, kappa=3, step=2, zdist=2, nodepervol=4, **kw)
    a = pnr_amd.Context(p, 0)
    ra = pnr_amd.advantra.run_pipeline(a, x, window=win)
    lo, hi = a.window
    k_lo, k_hi = ranks(x.size, 0, 3500)
    s = np.sort(x.ravel())
    assert (lo, hi) == (s[k_lo], s[k_hi])
    mapped = np_map(x, lo, hi)
    assert np.array_equal(a.get_volume(), mapped)
    b = pnr_amd.Context(p, 0)
    rb = pnr_amd.advantra.run_pipeline(b, mapped)
    for k in ("seeds_init", "seeds", "nodes", "links", "tree", "parent"):
        assert np.array_equal(ra[k], rb[k]), k
    assert len(ra["nodes"]) > 20
    a.close()
    b.close()


def _save16(path, x):
    from PIL import Image
    pages = [Image.frombytes("I;16", (x.shape[2], x.shape[1]), z.astype("<u2").tobytes()) for z in x]
    pages[0].save(path, save_all=True, append_images=pages[1:], compression=None)


def _save8(path, x):
    from PIL import Image
    pages = [Image.fromarray(z) for z in x]
    pages[0].save(path, save_all=True, append_images=pages[1:], compression=None)


def _cli(*args):
    return subprocess.run([CLI, *args], capture_output=True, text=True, timeout=600)


def test_cli_16bit_equals_mapped_8bit(tmp_path):
    """a 16-bit TIFF gives the SWC of the mapped 8-bit TIFF byte for byte, apart from the two comment lines of the window; channel 2
    of a 3-channel TIFF is that channel alone; --ranks 2 --share-gpu gives the one-GPU SWC"""
    img8 = synth.synth(64, 56, 32, seed=2)
    x = deep_stack(img8, 6)
    paras = "2,3 0 5 0.3 3 2 40 50 2 4 5".split()
    k_lo, k_hi = ranks(x.size, 100, 3500)
    s = np.sort(x.ravel())
    lo, hi = int(s[k_lo]), int(s[k_hi])
    outs = {}
    for name, flags, save, arr in (("deep", ("--saturate", "0.01,0.35"), _save16, x), ("flat", (), _save8, np_map(x, lo, hi)),
                                   ("fixed", ("--window", f"{lo},{hi}"), _save16, x)):
        d = tmp_path / name
        d.mkdir()
        tif = str(d / "stack.tif")
        save(tif, arr)
        r = _cli(*flags, "-f", "advantra_func", "-i", tif, "-p", *paras)
        assert r.returncode == 0, r.stderr
        outs[name] = open(tif + "_Advantra.swc").read()
    extra = f"#bits=16\n#window={lo},{hi}\n"
    assert extra in outs["deep"] and outs["deep"].replace(extra, "") == outs["flat"] and outs["fixed"] == outs["deep"]
    assert outs["flat"].count("\n") > 50 and "#channel=1\n" in outs["flat"]
    # channel 2 of a 3-channel (chunky) 16-bit TIFF = that channel alone, except for the #channel line
    rgb = np.stack([deep_stack(synth.synth(64, 56, 32, seed=s_), 7 + s_) for s_ in (1, 2, 3)], axis=-1)
    d = tmp_path / "rgb"
    d.mkdir()
    write_tiff(str(d / "rgb.tif"), list(rgb), spp=3)
    r = _cli("--channel", "2", "-f", "advantra_func", "-i", str(d / "rgb.tif"), "-p", *paras)
    assert r.returncode == 0, r.stderr
    _save16(str(d / "one.tif"), np.ascontiguousarray(rgb[..., 1]))
    r1 = _cli("-f", "advantra_func", "-i", str(d / "one.tif"), "-p", *paras)
    assert r1.returncode == 0, r1.stderr
    got, want = open(str(d / "rgb.tif") + "_Advantra.swc").read(), open(str(d / "one.tif") + "_Advantra.swc").read()
    assert "#channel=2\n" in got and got.replace("#channel=2\n", "#channel=1\n") == want
    # the sharded path on 16-bit input: every rank maps the whole stack once, slabs and stack share one window
    d = tmp_path / "ranks"
    d.mkdir()
    tif = str(d / "stack.tif")
    _save16(tif, x)
    r = _cli("--ranks", "2", "--share-gpu", "--saturate", "0.01,0.35", "-f", "advantra_func", "-i", tif, "-p", *paras)
    assert r.returncode == 0, r.stderr[-1500:]
    assert open(tif + "_Advantra.swc").read() == outs["deep"]


def test_int64_indexing_above_2_31_elements():
    """2048 x 1024 x 520 x 2 u16 (2^31 + 2^25 elements) on the device: the second channel, [min, max] and a fixed window, against
    the rule computed by torch in slabs"""
    import torch
    w, h, l, nchan = 2048, 1024, 520, 2
    n = w * h * l
    g = torch.Generator(device="cuda").manual_seed(9)
    t = torch.randint(0, 4096, (n * nchan,), dtype=torch.int32, device="cuda", generator=g)
    t[2 * (n - 1) + 1] = 65535  # the last voxel of channel 1 holds the maximum: read only with 64-bit element indices
    t[2 * (n - 7) + 1] = 3
    t16 = t.to(torch.int16)  # (bit pattern of the u16 samples)
    del t
    ch = t16[1::2].to(torch.int32) & 0xFFFF
    c = pnr_amd.Context(pnr_amd.make_params(sigmas=(2,)), 0)
    torch.cuda.synchronize()
    for win in (None, (100, 3000)):
        c.set_volume_device(t16.data_ptr(), (l, h, w), dtype=np.uint16, nchan=nchan, channel=1, window=win)
        lo, hi = c.window
        if win is None:
            assert (lo, hi) == (int(ch.min()), 65535)
        got = torch.from_numpy(c.get_volume().reshape(-1))
        step = 1 << 28
        for s in range(0, n, step):
            a = ch[s:s + step].clamp(lo, hi) - lo
            want = ((510 * a + (hi - lo)) // (2 * (hi - lo))).to(torch.uint8).cpu()
            assert torch.equal(got[s:s + step], want), (win, s)
    c.close()
