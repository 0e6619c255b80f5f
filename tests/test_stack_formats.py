"""The C++ loader (pnr_amd/host load_stack) on 16-bit, multi-channel and ImageJ hyperstack TIFFs and raw u16 stacks, through
`advantra_cli --info` (one JSON line of the kept channel, no GPU), and the CLI's refusals (CPU only: all of it runs before any
device call)."""
import json
import os
import struct
import subprocess
import numpy as np
import pytest
import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "pnr_amd", "host", "advantra_cli")
PARAS = "2 0 5 0.3 3 2 10 20 2 4 1".split()


def run(*args):
    if not os.path.exists(CLI):
        subprocess.run(["make", "-s", "-C", os.path.dirname(CLI)], check=True)
    return subprocess.run([CLI, *args], capture_output=True, text=True, timeout=300)


def write_tiff(path, planes, bps=16, spp=1, planar=1, fmt=None, desc=None, be=False):
    """a baseline TIFF, one page per plane, uncompressed: a plane is (h, w), (h, w, spp) chunky or (spp, h, w) planar (one strip per
    sample plane); values are written with `bps` bits in 8- or 16-bit containers"""
    e = ">" if be else "<"
    dt = np.dtype(e + ("u1" if bps <= 8 else "u2"))
    out = bytearray((b"MM" if be else b"II") + struct.pack(e + "HI", 42, 0))
    link = 4  # where the offset of the next IFD goes
    for a in planes:
        a = np.asarray(a)
        h, w = (a.shape[1], a.shape[2]) if planar == 2 else (a.shape[0], a.shape[1])
        strips = [a[c].astype(dt).tobytes() for c in range(spp)] if planar == 2 else [a.astype(dt).tobytes()]
        offs, cnts = [], []
        for st in strips:
            offs.append(len(out))
            cnts.append(len(st))
            out += st
        entries = [(256, 4, [w]), (257, 4, [h]), (258, 3, [bps] * spp), (259, 3, [1]), (262, 3, [2 if spp == 3 else 1]),
                   (273, 4, offs), (277, 3, [spp]), (278, 4, [h]), (279, 4, cnts), (284, 3, [planar])]
        if fmt is not None:
            entries.append((339, 3, [fmt] * spp))
        if desc is not None and link == 4:
            entries.append((270, 2, list(desc.encode() + b"\0")))
        entries.sort()
        fields = []
        for tag, typ, vals in entries:
            code = {2: "B", 3: "H", 4: "I"}[typ]
            raw = struct.pack(e + code * len(vals), *vals)
            if len(raw) <= 4:
                fields.append((tag, typ, len(vals), raw.ljust(4, b"\0")))
            else:
                if len(out) % 2:
                    out += b"\0"
                fields.append((tag, typ, len(vals), struct.pack(e + "I", len(out))))
                out += raw
        if len(out) % 2:
            out += b"\0"
        ifd = len(out)
        out[link:link + 4] = struct.pack(e + "I", ifd)
        out += struct.pack(e + "H", len(fields))
        for tag, typ, n, val in fields:
            out += struct.pack(e + "HHI", tag, typ, n) + val
        link = len(out)
        out += struct.pack(e + "I", 0)
    with open(path, "wb") as f:
        f.write(bytes(out))


def info(path, *flags):
    r = run("--info", *flags, "-i", str(path))
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout)


def expect(got, a, bits, channels, channel=1):
    l, h, w = a.shape
    want = {"w": w, "h": h, "l": l, "bits": bits, "channels": channels, "channel": channel, "min": int(a.min()), "max": int(a.max()),
            "sum": int(a.sum(dtype=np.uint64))}
    assert got == want, (got, want)


def stack16(shape, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 65536, shape, dtype=np.uint16)


@pytest.mark.parametrize("mode", ["I;16", "I;16B"])
def test_info_16bit_pil(tmp_path, mode):
    """16-bit TIFFs as PIL writes them, little- and big-endian"""
    from PIL import Image
    a = stack16((6, 13, 11), 1)
    pages = [Image.frombytes(mode, (11, 13), z.astype(">u2" if mode == "I;16B" else "<u2").tobytes()) for z in a]
    f = tmp_path / "s.tif"
    pages[0].save(f, save_all=True, append_images=pages[1:], compression=None)
    expect(info(f), a, 16, 1)


def test_info_8bit_rgb_every_channel(tmp_path):
    from PIL import Image
    rgb = np.random.default_rng(2).integers(0, 256, (5, 9, 7, 3), dtype=np.uint8)
    f = tmp_path / "rgb.tif"
    pages = [Image.fromarray(z, "RGB") for z in rgb]
    pages[0].save(f, save_all=True, append_images=pages[1:], compression=None)
    for c in (1, 2, 3):
        expect(info(f, "--channel", str(c)), rgb[..., c - 1], 8, 3, c)
    expect(info(f), rgb[..., 0], 8, 3, 1)


@pytest.mark.parametrize("be", [False, True])
def test_info_16bit_three_samples_chunky_and_planar(tmp_path, be):
    a = stack16((4, 10, 12, 3), 3)
    write_tiff(tmp_path / "chunky.tif", list(a), spp=3, planar=1, be=be)
    write_tiff(tmp_path / "planar.tif", [np.moveaxis(z, 2, 0) for z in a], spp=3, planar=2, be=be)
    for c in (1, 2, 3):
        expect(info(tmp_path / "chunky.tif", "--channel", str(c)), a[..., c - 1], 16, 3, c)
        expect(info(tmp_path / "planar.tif", "--channel", str(c)), a[..., c - 1], 16, 3, c)


def test_info_imagej_hyperstack(tmp_path):
    """ImageJ hyperstack, channels=2: the pages run channel-fastest"""
    a = stack16((5, 2, 9, 8), 4)  # z, c, y, x
    desc = "ImageJ=1.53t\nimages=10\nchannels=2\nslices=5\nhyperstack=true\nmode=composite\n"
    write_tiff(tmp_path / "hs.tif", [a[z, c] for z in range(5) for c in range(2)], desc=desc)
    for c in (1, 2):
        expect(info(tmp_path / "hs.tif", "--channel", str(c)), a[:, c - 1], 16, 2, c)
    r = run("--info", "--channel", "3", "-i", str(tmp_path / "hs.tif"))
    assert "Invalid channel number." in r.stderr


def test_info_raw_u16(tmp_path):
    a = stack16((3, 7, 10), 5)
    f = tmp_path / "s.raw"
    a.astype("<u2").tofile(f)
    expect(info(f, "--raw-type", "u16", "-d", "10,7,3"), a, 16, 1)
    expect(info(f, "-d", "10,7,6"), np.frombuffer(a.astype("<u2").tobytes(), np.uint8).reshape(6, 7, 10), 8, 1)  # u8: the same bytes
    r = run("--info", "--raw-type", "u16", "-d", "10,7,4", "-i", str(f))
    assert r.returncode == 1 and "raw file shorter" in r.stderr


def test_rejections(tmp_path):
    """what the loader and the flags refuse, each with its message; no SWC is written"""
    a = stack16((3, 8, 8), 6)
    cases = {
        "b12.tif": (dict(bps=12), "BitsPerSample = 12"),
        "float.tif": (dict(bps=32, fmt=3), "SampleFormat = 3"),
        "signed.tif": (dict(fmt=2), "SampleFormat = 2"),
        "frames.tif": (dict(desc="ImageJ=1.53t\nimages=3\nframes=3\n"), "frames=3"),
    }
    for name, (kw, msg) in cases.items():
        f = tmp_path / name
        planes = [z.astype(np.uint32) for z in a] if kw.get("bps") == 32 else list(a >> (4 if kw.get("bps") == 12 else 0))
        if kw.get("bps") == 32:  # 32-bit containers
            write_tiff_32(f, planes, **kw)
        else:
            write_tiff(f, planes, **kw)
        r = run("-f", "advantra_func", "-i", str(f), "-p", *PARAS)
        assert r.returncode == 0 and msg in r.stderr, (name, r.returncode, r.stderr)  # dofunc prints and returns, as for an unreadable image
        assert not os.path.exists(str(f) + "_Advantra.swc")
        assert run("--info", "-i", str(f)).returncode == 1
    rgb = np.random.default_rng(7).integers(0, 65536, (2, 6, 6, 3), dtype=np.uint16)
    write_tiff(tmp_path / "rgb16.tif", list(rgb), spp=3)
    r = run("--channel", "4", "-f", "advantra_func", "-i", str(tmp_path / "rgb16.tif"), "-p", *PARAS)
    assert r.returncode == 0 and "Invalid channel number." in r.stderr, r.stderr
    assert not os.path.exists(str(tmp_path / "rgb16.tif") + "_Advantra.swc")
    # flags: parse errors exit 1, like --exchange
    for flags, msg in ((("--saturate", "60,50"), "--saturate LO,HI"), (("--window", "9,9"), "--window LO,HI"),
                       (("--saturate", "0.12345,1"), "--saturate LO,HI"), (("--window", "0,65536"), "--window LO,HI"),
                       (("--channel", "0"), "--channel C"), (("--raw-type", "u12"), "--raw-type"),
                       (("--window", "1,2", "--saturate", "0,1"), "one of them")):
        r = run(*flags, "-f", "advantra_func", "-i", str(tmp_path / "rgb16.tif"), "-p", *PARAS)
        assert r.returncode == 1 and msg in r.stderr, (flags, r.stderr)
    # --window / --saturate on an 8-bit stack: a usage error
    from PIL import Image
    img = synth.synth(16, 12, 4, seed=1)
    f8 = str(tmp_path / "s8.tif")
    pages = [Image.fromarray(z) for z in img]
    pages[0].save(f8, save_all=True, append_images=pages[1:], compression=None)
    for flags in (("--window", "10,200"), ("--saturate", "0,0.35")):
        r = run(*flags, "-f", "advantra_func", "-i", f8, "-p", *PARAS)
        assert r.returncode == 1 and "need a 16-bit stack" in r.stderr, r.stderr


def write_tiff_32(path, planes, bps=32, fmt=3, **kw):
    """a float32 page layout (32-bit samples) for the refusal test"""
    e = "<"
    out = bytearray(b"II" + struct.pack(e + "HI", 42, 0))
    a = np.asarray(planes[0], np.float32)
    h, w = a.shape
    off = len(out)
    out += a.tobytes()
    ifd = len(out)
    out[4:8] = struct.pack(e + "I", ifd)
    entries = [(256, 4, 1, w), (257, 4, 1, h), (258, 3, 1, 32), (259, 3, 1, 1), (273, 4, 1, off), (277, 3, 1, 1), (278, 4, 1, h),
               (279, 4, 1, a.nbytes), (339, 3, 1, fmt)]
    out += struct.pack(e + "H", len(entries))
    for tag, typ, n, v in entries:
        out += struct.pack(e + "HHI", tag, typ, n) + (struct.pack(e + "HH", v, 0) if typ == 3 else struct.pack(e + "I", v))
    out += struct.pack(e + "I", 0)
    with open(path, "wb") as f:
        f.write(bytes(out))


def test_16bit_tiff_loads_then_needs_a_gpu(tmp_path):
    """a valid 16-bit TIFF gets past the loader (and a 2-channel one past the channel selection) to the device library, which has
    no CPU path: 'no HIP device', exit status 1, no SWC"""
    import torch
    if torch.cuda.is_available():
        pytest.skip("needs a machine without a GPU")
    a = stack16((4, 16, 20, 2), 8)
    f = tmp_path / "two.tif"
    write_tiff(f, list(a), spp=2)
    for flags in ((), ("--channel", "2", "--saturate", "0,0.35"), ("--window", "100,4000")):
        r = run(*flags, "-f", "advantra_func", "-i", str(f), "-p", *PARAS)
        assert r.returncode == 1 and "no HIP device" in r.stderr, (flags, r.returncode, r.stderr)
        assert not os.path.exists(str(f) + "_Advantra.swc")
