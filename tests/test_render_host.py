"""CPU: the render rule restated in numpy (render_ref.py) against closed forms, the host's work items (tap pnr_render_items) against the
restatement -- the boxes of a segment hold every voxel inside it, whatever the piece length and the sub-box size --, the volume writer
(tap pnr_test_write_tiff) read back by PIL and by advantra_cli --info, read_swc_nodes and the layout of the two new structs."""
import ctypes as C
import json
import os
import re
import subprocess
import numpy as np
import pytest
import pnr_amd
from pnr_amd import lib
import render_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "pnr_amd", "host", "advantra_cli")
F = np.float32
BALLS = {0: 1, 1: 7, 2.5: 81, 4: 257}  # lattice points with dx^2 + dy^2 + dz^2 <= R^2
DISK2, BALL2 = 13, 33                  # ... of the disk and the ball of radius 2


def test_restatement_balls_and_capsule():
    for R, count in BALLS.items():
        L = render_ref.render([[8, 8, 8]], [R], [-1], (17, 17, 17))
        assert int((L > 0).sum()) == count and set(np.unique(L)) <= {0, 1}, R
    L = render_ref.render([[3, 4, 5]], [0], [-1], (9, 9, 9))
    assert np.argwhere(L > 0).tolist() == [[5, 4, 3]]  # (z, y, x)
    # a capsule of radius 2 along x from x = 5 to x = 15: eleven disks and the two half balls beyond the ends; node 1 draws it (label 2)
    # except where the ball of node 0 (label 1) was first
    L = render_ref.render([[5, 8, 8], [15, 8, 8]], [2, 2], [-1, 0], (17, 17, 21))
    assert int((L > 0).sum()) == 11 * DISK2 + (BALL2 - DISK2)
    assert int((L == 1).sum()) == BALL2 and L[8, 8, 10] == 2 and L[8, 8, 3] == 1 and L[8, 8, 17] == 2 and L[8, 8, 18] == 0
    # zscale 2: plane z is the point 2 z, so a ball of radius 2 around plane 4 holds the planes 3..5 only
    L = render_ref.render([[8, 8, 4]], [2], [-1], (9, 17, 17), zscale=2)
    assert sorted(set(np.argwhere(L > 0)[:, 0].tolist())) == [3, 4, 5] and int((L > 0).sum()) == DISK2 + 2


def random_pairs(rng, shape, pairs, zscale):
    """`pairs` edges (parent, child), ends up to 10 voxels outside the grid, radii 0..12 (mostly small)"""
    l, h, w = shape
    n = 2 * pairs
    xyz = np.stack([rng.uniform(-10, w + 10, n), rng.uniform(-10, h + 10, n), rng.uniform(-10 / zscale, l + 10 / zscale, n)], 1).astype(F)
    xyz[::7] = np.round(xyz[::7])
    radius = np.where(rng.random(n) < 0.8, rng.uniform(0, 3, n), rng.uniform(3, 12, n)).astype(F)
    radius[::5] = 0
    parent = np.where(np.arange(n) % 2 == 0, -1, np.arange(n) - 1).astype(np.int32)
    return xyz, radius, parent


@pytest.mark.parametrize("zscale", [1, 2, 2.5, 4])
def test_items_cover_every_inside_voxel(zscale):
    rng = np.random.default_rng(int(zscale * 10))
    shape = (14, 26, 30)
    xyz, radius, parent = random_pairs(rng, shape, 30, zscale)
    x = render_ref.scaled(xyz, zscale)
    rr = render_ref.radii(radius)
    want = [render_ref.inside(shape, x[i], x[i if parent[i] < 0 else parent[i]], rr[i], rr[i if parent[i] < 0 else parent[i]], zscale) for i in range(len(x))]
    assert sum(int(m.sum()) for m in want) > 0  # the check is not about empty sets
    for piece, box in ((1, 0), (4, 0), (16, 0), (16, 50), (0, 1), (0, 0)):
        items = pnr_amd.render_items(xyz, radius, parent, shape, zscale=zscale, piece=piece, box=box)
        assert (items[:, 1:4] >= 0).all() and (items[:, 4:7] >= items[:, 1:4]).all() and (items[:, 4:7] < np.array(shape[::-1])).all()
        assert (np.diff(items[:, 0]) >= 0).all() and items[:, 0].min() >= 0 and items[:, 0].max() < len(x)
        vol = np.prod(items[:, 4:7] - items[:, 1:4] + 1, axis=1)
        if box:
            assert vol.max() <= box
        for i in range(len(x)):
            got = np.zeros(shape, bool)
            for _, x0, y0, z0, x1, y1, z1 in items[items[:, 0] == i]:
                got[z0:z1 + 1, y0:y1 + 1, x0:x1 + 1] = True
            assert not (want[i] & ~got).any(), (piece, box, i)


def test_items_follow_a_long_edge():
    """a radius-2 diagonal edge of length 200 in 256^3: the boxes total less than 5 % of the edge's own bounding box"""
    d = 200 / np.sqrt(3)
    a, b = np.array([20, 20, 20], F), np.array([20 + d, 20 + d, 20 + d], F)
    items = pnr_amd.render_items([a, b], [2, 2], [-1, 0], (256, 256, 256))
    edge = items[items[:, 0] == 1]
    total = int(np.prod(edge[:, 4:7] - edge[:, 1:4] + 1, axis=1).sum())
    bbox = float(np.prod(np.ceil(b + 2) - np.floor(a - 2) + 1))
    print(f"boxes {total} voxels = {100 * total / bbox:.2f} % of the bounding box ({int(bbox)}), {len(edge)} items")
    assert len(edge) >= 13 and total < 0.05 * bbox


def test_items_arguments_and_empty_cases():
    assert len(pnr_amd.render_items(np.zeros((0, 3), F), [], [], (4, 4, 4))) == 0
    assert len(pnr_amd.render_items([[100, 100, 100]], [3], [-1], (8, 8, 8))) == 0  # out of reach of the grid
    assert len(pnr_amd.render_items([[-2, 3, 3]], [3], [-1], (8, 8, 8))) == 1        # centred outside, reaching in
    assert len(pnr_amd.render_items([[3, 3, 5]], [1], [-1], (1, 8, 8))) == 0         # 2-D: only z = 0 exists
    for bad in (dict(xyz=[[np.nan, 0, 0]]), dict(radius=[-1]), dict(radius=[np.inf]), dict(parent=[1]), dict(zscale=0), dict(rscale=-1), dict(radd=np.inf),
                dict(radius=[1025]), dict(shape=(0, 4, 4))):
        kw = dict(xyz=[[1, 1, 1]], radius=[1], parent=[-1], shape=(4, 4, 4))
        kw.update(bad)
        with pytest.raises(pnr_amd.PnrError, match="error -1"):
            pnr_amd.render_items(**kw)


def info(path):
    r = subprocess.run([CLI, "--info", "-i", str(path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout)


@pytest.mark.parametrize("shape", [(3, 5, 7), (1, 9, 11), (20, 48, 64)])
def test_tiff_writer_reads_back(tmp_path, shape):
    from PIL import Image
    rng = np.random.default_rng(shape[0])
    img = rng.integers(0, 256, shape, dtype=np.uint8)
    path = tmp_path / "out.tif"
    lib.write_tiff(path, img)
    assert os.listdir(tmp_path) == ["out.tif"]  # the temporary file is gone
    with Image.open(path) as im:
        assert im.n_frames == shape[0]
        pages = []
        for z in range(im.n_frames):
            im.seek(z)
            pages.append(np.array(im))
    assert np.array_equal(np.stack(pages), img)
    l, h, w = shape
    assert info(path) == {"w": w, "h": h, "l": l, "bits": 8, "channels": 1, "channel": 1, "min": int(img.min()), "max": int(img.max()), "sum": int(img.sum())}
    lib.write_tiff(tmp_path / "out.raw", img)
    assert open(tmp_path / "out.raw", "rb").read() == img.tobytes()


def test_tiff_writer_refuses_4gib_from_the_dimensions(tmp_path):
    path = tmp_path / "big.tif"
    rc = lib.load().pnr_test_write_tiff(os.fsencode(path), None, 2048, 2048, 1024)  # 4 GiB of voxels: no image is passed at all
    assert rc == -1 and "4 GiB" in lib.load().pnr_last_error().decode() and os.listdir(tmp_path) == []


def test_read_swc_nodes(tmp_path):
    f = tmp_path / "t.swc"
    f.write_text("# a comment\n3 2 1.5 2 3 0.75 -1\n\n7.0 3 4 5 6 2 3\n9 6 0 0 1 0 42\n")
    xyz, radius, typ, parent, ids = pnr_amd.read_swc_nodes(f)
    assert xyz.dtype == F and radius.dtype == F and typ.dtype == np.int32 and parent.dtype == np.int32 and ids.dtype == np.int64
    assert xyz.tolist() == [[1.5, 2, 3], [4, 5, 6], [0, 0, 1]] and radius.tolist() == [0.75, 2, 0] and typ.tolist() == [2, 3, 6]
    assert parent.tolist() == [-1, 0, -1] and ids.tolist() == [3, 7, 9]
    a, b, c = pnr_amd.read_swc(f)
    assert np.array_equal(a, xyz) and np.array_equal(b, parent) and np.array_equal(c, ids)


def test_struct_layout_matches_header():
    hdr = open(os.path.join(ROOT, "include", "pnr_hip.h")).read()
    ctype = {"float": C.c_float, "int32_t": C.c_int32, "int64_t": C.c_int64, "double": C.c_double}
    for name, cls in (("pnr_render_opts", lib.RenderOpts), ("pnr_coverage", lib.Coverage)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), hdr, re.S).group(1)
        fields = []
        for decl in filter(None, (d.strip() for d in body.split(";"))):
            t, names = decl.split(None, 1)
            fields += [(n.strip(), ctype[t]) for n in names.split(",")]
        assert fields == list(cls._fields_), name
    assert C.sizeof(lib.RenderOpts) == 16 and C.sizeof(lib.Coverage) == 6 * 8 + 8 + 3 * 8
    assert lib.PNR_RENDER_MAX_N == 1 << 22 and "#define PNR_RENDER_MAX_N (1 << 22)" in hdr and "#define PNR_RENDER_MAX_R 1024" in hdr
