"""GPU parity of the soma path (somaradius > 0) through the C ABI: eroded + blurred stack, threshold, soma
nodes and label map vs the oracle (bit-exact: bytes, integers and f32 running means in the same order), then the whole
path -- seeds in the soma dropped, traces that reach the soma stopped and linked to its node, final tree list."""
import numpy as np
import pytest
import orc
import synth
import pnr_amd
from pnr_amd import lib

pytestmark = pytest.mark.gpu


def _stack(shape=(32, 56, 64), seed=2, somas=((20, 28, 16, 6), (48, 20, 14, 5))):
    l, h, w = shape
    return synth.add_somas(synth.synth(w, h, l, seed=seed), somas)


def _soma_vs_oracle(oracle, img, rad):
    """pnr_soma on `img` equals the oracle's soma path: eroded + blurred stack, threshold, the label map as (voxel, label) pairs in
    raster order and the four node columns; the threshold is the one of E8's histogram with every voxel counted once.  Returns
    the oracle's (E8, threshold, node columns, foreground voxels)"""
    E8o, tho, smapo, n4o = orc.soma_extract(oracle, img, rad)
    c = pnr_amd.Context(pnr_amd.make_params(sigmas=[2.0], somaradius=rad, np_=20, ni=5), 0)
    c.set_volume(img)
    s = c.soma(want_e8=True)
    c.close()
    assert np.array_equal(s["E8"], E8o)
    assert s["threshold"] == tho
    hist = np.bincount(s["E8"].reshape(-1), minlength=256).astype(np.int64)
    assert hist.sum() == img.size and oracle.orc_maxentropy_hist(hist) == s["threshold"]
    assert oracle.orc_maxentropy_th(np.ascontiguousarray(s["E8"]).reshape(-1), img.size) == s["threshold"]
    assert len(s["nodes"]) == len(n4o)
    got4 = np.stack([s["nodes"][k] for k in ("x", "y", "z", "sig")], -1) if len(n4o) else np.zeros((0, 4), np.float32)
    assert np.array_equal(got4, n4o)
    assert np.all(s["nodes"]["type"] == 1) and np.all(s["nodes"]["corr"] == -np.finfo(np.float32).max)
    fg = np.flatnonzero(smapo.reshape(-1) > 0)
    assert np.array_equal(s["vox"], fg) and np.array_equal(s["lab"], smapo.reshape(-1)[fg])
    return E8o, tho, n4o, fg


@pytest.mark.parametrize("shape,rad,somas", [((32, 56, 64), 3, ((20, 28, 16, 6), (48, 20, 14, 5))), ((9, 20, 23), 2, ((10, 10, 4, 4),)),
                                             ((24, 40, 48), 4, ())])
def test_soma_extraction_vs_oracle(oracle, shape, rad, somas):
    img = _stack(shape, 3, somas)
    E8o, tho, n4o, fg = _soma_vs_oracle(oracle, img, rad)
    if somas:
        assert len(n4o) >= 1 and len(fg) > 20


@pytest.mark.parametrize("rad", [1, 5, 6, 8, 21])
def test_soma_radii_vs_oracle(oracle, rad):
    """the radii the other cases leave out, up to the largest validate() accepts, on 130 x 70 x 12: three x tiles of
    gauss_y_trunc_hist (the last two columns wide), three ballots a row in row_count / row_compact, and -- radii 6, 12, 18 and 24
    of the Gaussian at somaradius 2, 4, 6, 8 being the templated ones -- at 6 and 8 an interior, whole-dword tile of
    gauss_x_u8_t<18> / <24>, which Frangi's own dispatch never hands these radii to.  Two of the three cell bodies are cut by the
    border of the stack"""
    img = synth.add_somas(synth.synth(130, 70, 12, seed=2), ((5, 5, 3, rad + 3), (100, 40, 6, rad + 4), (127, 66, 10, rad + 2)))
    E8o, tho, n4o, fg = _soma_vs_oracle(oracle, img, rad)
    assert len(n4o) >= 2 and len(fg) > 0


@pytest.mark.parametrize("rad", [2, 4])
def test_soma_templated_x_pass_interior_tile(oracle, rad):
    """gauss_x_u8_t<6> / <12> (somaradius 2 / 4; Frangi runs these radii in its fused kernels) on a stack wide enough for an
    interior tile that reads whole dwords, with a ragged last tile and a body on the right border"""
    img = synth.add_somas(synth.synth(130, 70, 12, seed=2), ((5, 5, 3, rad + 3), (100, 40, 6, rad + 4), (127, 66, 10, rad + 2)))
    E8o, tho, n4o, fg = _soma_vs_oracle(oracle, img, rad)
    assert len(n4o) >= 2 and len(fg) > 0


@pytest.mark.parametrize("rad", [2, 4, 6, 8])
def test_soma_templated_x_pass_random_bytes(oracle, rad):
    """the four radii of gauss_x_u8_t on random bytes of 90 and more: the eroded stack is nowhere zero, so every tile of the x pass
    -- border, interior (whole dwords) and the ragged last one -- and its second, one-row tile of rows (5 x 13 = 65 rows) sums data"""
    img = np.random.default_rng([9, rad]).integers(90, 256, (5, 13, 130), dtype=np.uint8)
    E8o, tho, n4o, fg = _soma_vs_oracle(oracle, img, rad)
    assert E8o.min() > 0 and len(np.unique(E8o)) > 3


@pytest.mark.parametrize("shape,rad", [((3, 7, 9), 8), ((2, 33, 40), 21)])
def test_soma_window_wider_than_stack(oracle, shape, rad):
    """erosion and blur windows wider than the stack in x and in y: most taps are clamped ones.  Each plane has a positive minimum of
    its own, so the eroded stack is not empty -- but at radius 21 (127 taps, the running sum cut to a byte after each) the plane whose
    minimum is 40 blurs to 0: every product is below 1"""
    l = shape[0]
    img = np.stack([np.random.default_rng([4, z]).integers(40 + 30 * z, 256, shape[1:], dtype=np.uint8) for z in range(l)])
    E8o, tho, n4o, fg = _soma_vs_oracle(oracle, img, rad)
    assert E8o.max() > 0 and len({int(E8o[z].max()) for z in range(l)}) == l


@pytest.mark.parametrize("w", [63, 64, 65, 129])
def test_soma_tile_edges(oracle, w):
    """widths around one and two x tiles of gauss_y_trunc_hist / one and two ballots of the row kernels, 33 rows: one row in the
    second y tile, and a body on the lower right corner so that this row and the last column are foreground"""
    img = synth.add_somas(synth.synth(w, 33, 3, seed=5), ((w - 4, 31, 1, 6), (12, 10, 1, 5)))
    E8o, tho, n4o, fg = _soma_vs_oracle(oracle, img, 2)
    smap_fg = np.zeros(img.size, bool)
    smap_fg[fg] = True
    smap_fg = smap_fg.reshape(img.shape)
    assert len(n4o) >= 1 and smap_fg[:, 32, :].any() and smap_fg[:, :, w - 1].any()


def _flat(value):
    return np.full((4, 40, 70), value, np.uint8)


def _salt_and_pepper():
    return (np.random.default_rng(8).integers(0, 2, (4, 40, 70)) * 255).astype(np.uint8)


@pytest.mark.parametrize("name,make,e8,regions", [("zeros", lambda: _flat(0), 0, 0), ("full", lambda: _flat(255), 246, 1),
                                                  ("grey", lambda: _flat(37), 31, 1), ("salt_and_pepper", _salt_and_pepper, 0, 0)])
def test_soma_without_contrast(oracle, name, make, e8, regions):
    """stacks whose eroded + blurred form is one value.  The y pass cuts its running sum to a byte at every tap, so a stack of
    255s blurs to 246 and one of 37s to 31; the histogram is one bin, the threshold 0, and everything above it -- the whole stack,
    or nothing -- is one region"""
    img = make()
    E8o, tho, n4o, fg = _soma_vs_oracle(oracle, img, 2)
    assert tho == 0 and np.all(E8o == e8) and len(n4o) == regions
    assert len(fg) == (img.size if regions else 0)


def test_soma_radius_bound():
    """21 is the largest somaradius (Gaussian radius 63 of at most 64 taps a side, test_soma_radii_vs_oracle runs it); 22 is refused"""
    with pytest.raises(lib.PnrError, match="somaradius 22 too large"):
        pnr_amd.Context(pnr_amd.make_params(sigmas=[2.0], somaradius=22, np_=20, ni=5), 0)


def test_no_soma_when_radius_zero():
    img = _stack()
    c = pnr_amd.Context(pnr_amd.make_params(sigmas=[2.0], somaradius=0, np_=20, ni=5), 0)
    c.set_volume(img)
    s = c.soma()
    assert len(s["nodes"]) == 0 and len(s["vox"]) == 0


def test_filter_needs_soma_first():
    img = _stack()
    c = pnr_amd.Context(pnr_amd.make_params(sigmas=[2.0], somaradius=3, np_=20, ni=5), 0)
    c.set_volume(img)
    c.frangi()
    with pytest.raises(lib.PnrError, match="pnr_soma"):
        c.score_filter_sort(c.extract_seeds())


@pytest.mark.parametrize("driver", ["phased", "persistent"])
def test_end_to_end_with_soma_vs_oracle(oracle, driver):
    """somaradius = 3 on a stack with two cell bodies: oracle = soma path + Frangi + seeds (those inside the soma dropped,
    Advantra_plugin.cpp:2561-2564) + tracker + replay with the soma stop (tracker.cpp:858-869) + reconstruct chain."""
    img = _stack()
    sigs, zdist, np_, ni, rad = [2.0, 3.0], 2.0, 40, 25, 3
    E8o, tho, smapo, n4o = orc.soma_extract(oracle, img, rad)
    assert len(n4o) >= 1
    J, jmin, jmax, Vx, Vy, Vz = orc.frangi3d(oracle, img, sigs, zdist)
    so = orc.extract_seeds(oracle, 5, orc.j8(oracle, J, jmin, jmax), Vx, Vy, Vz)
    l, h, w = img.shape
    vox = np.round(so[:, 2]).astype(np.int64) * w * h + np.round(so[:, 1]).astype(np.int64) * w + np.round(so[:, 0]).astype(np.int64)
    keep = smapo.reshape(-1)[vox] == 0
    assert (~keep).sum() > 0  # some seeds sit inside a soma
    so = so[keep]
    To = orc.Tracker(oracle, sigs, 2, np_, ni, 3.0, 0.3, zdist=zdist)
    corr, _ = To.zncc(img, so[:, :6])
    so[:, 7] = corr
    so = so[corr >= 0.3]
    so = so[np.argsort(-so[:, 7], kind="stable")]
    Tn, xcs = [], []
    for sd in so:
        for sgn in (1, -1):
            q = sd[:6].copy(); q[3:] *= sgn
            t, st, xco, *_ = To.trace(img, q)
            Tn.append(t); xcs.append(xco)
    nodes_o, links_o, nt_o = orc.replay(oracle, so, np.array(Tn, np.int32), np.stack(xcs), ni, img.shape, 4, 1, smap=smapo, soma4=n4o)
    tree_o, par_o = orc.reconstruct(oracle, nodes_o, links_o)

    p = pnr_amd.make_params(sigmas=sigs, somaradius=rad, np_=np_, ni=ni, zdist=zdist)
    c = pnr_amd.Context(p, 0)
    c.set_smc_driver(driver)
    res = pnr_amd.advantra.run_pipeline(c, img)
    assert len(res["seeds"]) == len(so)
    nodes, links = res["nodes"], res["links"]
    assert len(nodes) == len(nodes_o) and np.array_equal(links, links_o)
    for k in nodes.dtype.names:
        assert np.array_equal(nodes[k], nodes_o[k]), k
    nsoma = len(n4o)
    assert np.all(nodes["type"][1:1 + nsoma] == 1)
    soma_links = ((links <= nsoma) & (links >= 1)).any(1).sum()
    print("soma nodes", nsoma, "links into a soma", soma_links, "nodes", len(nodes))
    assert soma_links > 0  # a trace reached a cell body and was linked to it
    assert len(res["tree"]) == len(tree_o) and np.array_equal(res["parent"], par_o)
    for k in tree_o.dtype.names:
        assert np.array_equal(res["tree"][k], tree_o[k]), k
    # the one-shot form (trace everything, one replay) gives the same graph
    T, stop, xc, _ = c.trace_batch(res["seeds"])
    n1, l1, _ = c.replay(res["seeds"], T, xc)
    assert len(n1) == len(nodes) and np.array_equal(l1, links)


@pytest.mark.parametrize("name", ["soma_64x56x32_r3", "soma_23x20x9_r2"])
def test_soma_filters_vs_golden(name):
    """eroded + blurred stack against the reference's own Frangi::imerode / u8 Frangi::imgaussian (tests/golden)"""
    import os
    g = dict(np.load(os.path.join(os.path.dirname(__file__), "golden", name + ".npz")))
    c = pnr_amd.Context(pnr_amd.make_params(sigmas=[2.0], somaradius=int(g["rad"]), np_=20, ni=5), 0)
    c.set_volume(g["img"])
    s = c.soma(want_e8=True)
    assert np.array_equal(s["E8"], g["blurred"])


# ---- the sparse stack above 2^31 voxels (tests/bigtrace.py) and its sibling ----
def _sparse_soma_context(shape):
    import bigtrace
    return bigtrace.open_stack(shape, dict(bigtrace.PARAMS, somaradius=3))


@pytest.fixture(scope="module")
def dark_stack():
    """2048 x 2048 x 536, zero but for two blocks of tubes, borrowed by a context with somaradius 3; the two tests below share it, so
    that the second runs on the context that refused the call"""
    import torch
    import bigtrace
    t, c = _sparse_soma_context(bigtrace.SHAPE)
    S = dict(c=c, error=None)
    yield S
    c.close()
    del t
    torch.cuda.empty_cache()


def _refused(S):
    if S["error"] is None:
        with pytest.raises(lib.PnrError) as e:
            S["c"].soma()
        S["error"] = str(e.value)
    return S["error"]


def test_soma_refuses_a_histogram_bin_of_2_31(dark_stack):
    """bin 0 of the eroded + blurred stack's histogram holds more than 2^31 voxels, which the maximum-entropy rule would read as a
    negative `int` (threshold_rule.cpp; the reference's `int hist[]`): pnr_soma refuses it by name and leaves no soma map behind"""
    import re
    import bigtrace
    shape = bigtrace.SHAPE
    n_vox = int(np.prod(shape, dtype=np.int64))
    text = _refused(dark_stack)
    m = re.search(r"pnr_soma: maxentropy needs every bin below 2\^31, bin 0 holds (\d+)", text)
    assert m and "error -1" in text, text
    assert max(2**31, n_vox - sum(B.size for _, B in bigtrace.blocks(shape))) <= int(m.group(1)) < n_vox, "all but some voxels of the blocks"
    assert not dark_stack["c"].have_soma()


def test_context_goes_on_after_the_refused_soma(dark_stack, oracle):
    """the context that refused pnr_soma stays usable: its Frangi gives the bytes that test_gpu_bigtrace.py holds against the oracle"""
    import bigtrace
    c = dark_stack["c"]
    _refused(dark_stack)
    fw = bigtrace.frangi_reference(oracle, bigtrace.SHAPE)
    assert not c.have_soma() and c.frangi() == (fw["jmin"], fw["jmax"])
    bigtrace.check_frangi(c, fw, whole_j8=False)


def test_soma_of_the_sparse_sibling_vs_oracle(oracle):
    """the same blocks on 160 x 96 x 72, the same call: every bin fits, and the soma path equals the oracle's"""
    import torch
    import bigtrace
    shape = bigtrace.SMALL
    img = bigtrace.host_stack(shape)
    E8o, tho, smapo, n4o = orc.soma_extract(oracle, img, 3)
    t, c = _sparse_soma_context(shape)
    s = c.soma(want_e8=True)
    assert c.have_soma() and np.array_equal(s["E8"], E8o) and s["threshold"] == tho
    hist = np.bincount(E8o.reshape(-1), minlength=256).astype(np.int64)
    assert hist[0] > 0.9 * img.size and oracle.orc_maxentropy_hist(hist) == tho
    fg = np.flatnonzero(smapo.reshape(-1) > 0)
    assert np.array_equal(s["vox"], fg) and np.array_equal(s["lab"], smapo.reshape(-1)[fg]) and len(s["nodes"]) == len(n4o)
    if len(n4o):
        assert np.array_equal(np.stack([s["nodes"][k] for k in ("x", "y", "z", "sig")], -1), n4o)
    c.close()
    del t
    torch.cuda.empty_cache()
